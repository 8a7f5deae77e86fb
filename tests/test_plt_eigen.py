"""CPU: the PLT eigenmode table (csrc/zd_kernels_plt.hip).  Pins the yardstick tests/plt_eigen_ref.py against what the definition
must give (sum rule, independence of the Ewald splitting, fluid limit, two closed points of the zone, cubic symmetry), and the host
side of the feature: the parameter keys ZD_PLT_compute_ppd / ZD_PLT_write_filename and the file writer zd_write_eigmodes."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import plt_eigen_ref as ref
from conftest import WMAP

N = 128
# axes, faces, edges, the corner, the neighbours of k = 0, and modes of no symmetry
MODES = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (64, 0, 0), (0, 64, 0), (0, 0, 64), (64, 64, 0), (64, 0, 64), (0, 64, 64), (64, 64, 64),
         (1, 1, 0), (1, 1, 1), (3, 3, 0), (17, 17, 17), (64, 5, 0), (64, 64, 9), (5, -7, 30), (-23, 41, 2), (12, 50, 63), (-64 + 1, 33, 7),
         (2, -1, 0), (31, 32, 33), (-40, -40, 11), (64, -13, 64)]


def test_sum_rule():
    """tr D = 1 at every wavevector (Kohn)"""
    for m in MODES:
        assert abs(np.trace(ref.matrix(m, N)) - 1.0) <= 1e-13, m


def test_independent_of_the_ewald_splitting():
    for m in MODES:
        d = np.abs(ref.matrix(m, N, 2.0, 4) - ref.matrix(m, N, 1.5, 5)).max()
        assert d <= 1e-13, (m, d)


def test_fluid_limit():
    """D -> khat khat as k -> 0; the deviation is O(k^2): 1.4e-6 at m = (1, 2, 3) / 4096"""
    m = np.array([1.0, 2.0, 3.0])
    kh = m / np.sqrt((m * m).sum())
    dev = [np.abs(ref.matrix(m, n) - np.outer(kh, kh)).max() for n in (1024, 4096)]
    assert 1.3e-6 < dev[1] < 1.6e-6
    assert 15.0 < dev[0] / dev[1] < 17.0  # 4^2
    e, lam, _gap, _margin, _w = ref.mode(m, 4096)
    assert abs(lam - 1.0) < 1e-5 and np.abs(e - kh).max() < 1e-5


def test_zone_face_and_corner():
    w = np.linalg.eigvalsh(ref.matrix((64, 0, 0), N))
    assert np.abs(w - [-0.05211778, -0.05211778, 1.10423556]).max() <= 1e-8
    e, lam, gap, _margin, _w = ref.mode((64, 0, 0), N)
    assert np.abs(e - [1, 0, 0]).max() <= 1e-12 and abs(lam - 1.10423556) <= 1e-8 and gap > 1.0
    D = ref.matrix((64, 64, 64), N)
    assert np.abs(D - np.eye(3) / 3).max() <= 1e-8
    e, lam, gap, _margin, _w = ref.mode((64, 64, 64), N)  # a degenerate space: e is khat, not what the solver returns
    assert np.abs(e - np.ones(3) / np.sqrt(3)).max() <= 1e-12 and abs(lam - 1 / 3) <= 1e-8 and gap == np.inf


def test_cubic_symmetry():
    """permuting or reflecting m permutes or reflects e; lambda is unchanged"""
    for m in [(5, -7, 30), (12, 50, 63), (3, 3, 0), (64, 5, 0)]:
        e0, lam0, _g, _mg, _w = ref.mode(m, N)
        for perm in itertools.permutations(range(3)):
            for sign in itertools.product((1, -1), repeat=3):
                m2 = tuple(sign[a] * m[perm[a]] for a in range(3))
                if -N // 2 in m2:
                    continue  # -n/2 is not a wavenumber of the table: index n/2 holds +n/2
                e, lam, _g, _mg, _w = ref.mode(m2, N)
                assert abs(lam - lam0) <= 1e-13, (m, m2)
                assert np.abs(e - [sign[a] * e0[perm[a]] for a in range(3)]).max() <= 1e-9, (m, m2)


def test_whole_small_table():
    """every entry of a table of 8 points: unit vectors on the k side, lambda inside the band, entry 0"""
    T, gap, margin = ref.table(8)
    assert np.array_equal(T[0, 0, 0], [0, 0, 0, 1])
    norm = np.sqrt((T[..., :3] ** 2).sum(-1))
    norm[0, 0, 0] = 1.0
    assert np.abs(norm - 1).max() <= 1e-14
    assert T[..., 3].min() > 0.32 and T[..., 3].max() < 1.105
    assert T[4, 0, 0, 3] == pytest.approx(1.10423556, abs=1e-8) and np.abs(T[4, 0, 0, :3] - [1, 0, 0]).max() <= 1e-12  # index n/2 is +n/2
    assert np.all((gap < ref.GROUP_TOL) | (gap > 1e-3)) and margin.min() > 1e-3


# ---- the host side of the feature ----------------------------------------------------------------------------------------------
PAR = """BoxSize = 720
CPD = 5
ICFormat = "RVdoubleZel"
InitialConditionsDirectory = "%(out)s"
InitialRedshift = 49
NP = 262144
ZD_NumBlock = 2
ZD_Pk_filename = "%(pk)s"
ZD_Pk_norm = 8.0
ZD_Pk_scale = 1.0
ZD_Pk_sigma = 0.0210839935761
ZD_Pk_smooth = 0.0
ZD_Seed = 12346
ZD_Version = 2
ZD_qPLT = 1
"""


@pytest.fixture()
def zd():
    import zeldovich_plt_amd.api as api
    api.load_library()
    return api


def _par(tmp_path, extra):
    par = tmp_path / "t.par"
    par.write_text(PAR % dict(out=tmp_path / "ic", pk=WMAP) + extra)
    return str(par)


def _read(zd, tmp_path, extra):
    return zd.params_from_file(_par(tmp_path, extra))


def test_reader_accepts_a_computed_table(zd, tmp_path):
    p, s = _read(zd, tmp_path, 'ZD_PLT_compute_ppd = 32\nZD_PLT_write_filename = "%s"\n' % (tmp_path / "eig32"))
    assert p.qPLT == 1 and s.PLT_compute_ppd == 32 and s.PLT_filename == b""
    assert zd.param_file_string(str(tmp_path / "t.par"), "ZD_PLT_write_filename") == str(tmp_path / "eig32")
    p, s = _read(zd, tmp_path, 'ZD_PLT_filename = "some_file"\n')  # as before
    assert s.PLT_compute_ppd == 0 and s.PLT_filename == b"some_file"
    assert zd.param_file_string(str(tmp_path / "t.par"), "ZD_PLT_write_filename") == ""
    assert zd.param_file_string(str(tmp_path / "t.par"), "ICFormat") == "RVdoubleZel"
    with pytest.raises(ValueError):
        zd.param_file_string(str(tmp_path / "absent.par"), "ICFormat")


def test_the_strings_struct_keeps_its_size(zd):
    """PLT_compute_ppd fills the four bytes of padding that ended zd_param_strings: a caller built against the earlier header passes a
    struct of the same size"""
    S = zd.ZdParamStrings
    assert S.PLT_compute_ppd.offset == S.SelfCheck_filename.offset + 1024 and C.sizeof(S) == S.PLT_compute_ppd.offset + 4


@pytest.mark.parametrize("extra,words", [
    ('ZD_PLT_compute_ppd = 32\nZD_PLT_filename = "some_file"\n', "both"),
    ("ZD_PLT_compute_ppd = 7\n", "ZD_PLT_compute_ppd = 7"),
    ("ZD_PLT_compute_ppd = 1024\n", "ZD_PLT_compute_ppd = 1024"),
    ("ZD_PLT_compute_ppd = 2\n", "ZD_PLT_compute_ppd = 2"),
    ("", "PLT_filename"),  # neither key: the reference's assertion, as before
])
def test_reader_refusals(zd, tmp_path, capfd, extra, words):
    with pytest.raises(ValueError):
        _read(zd, tmp_path, extra)
    err = capfd.readouterr().err
    assert "Invalid Parameters given" in err and words in err


def test_write_load_round_trip(zd, tmp_path):
    """zd_write_eigmodes is the inverse of zd_load_eigmodes, bit for bit (NaN payloads, signed zeros and denormals included)"""
    n = 6
    rng = np.random.default_rng(11)
    t = rng.standard_normal((n, n, n // 2 + 1, 4))
    t.view(np.uint64)[0, 0, 0] = [0x7FF8000000000123, 0x8000000000000000, 0x0000000000000001, 0xFFF0000000000000]
    f = tmp_path / "eig6"
    zd.write_eigenmodes(str(f), t)
    raw = f.read_bytes()
    assert len(raw) == 4 + t.nbytes and np.frombuffer(raw[:4], dtype="<i4")[0] == n and raw[4:] == t.tobytes()
    back = zd.load_eigenmodes(str(f))
    assert back.shape == t.shape and np.array_equal(back.view(np.uint64), t.view(np.uint64))
    # refusals: no table, a path that cannot be opened
    L = zd.load_library()
    assert L.zd_write_eigmodes(os.fsencode(str(tmp_path / "x")), None, n) != 0
    assert L.zd_write_eigmodes(os.fsencode(str(tmp_path / "no_such_dir" / "x")), t.ctypes.data, n) != 0
    with pytest.raises(ValueError):
        zd.write_eigenmodes(str(f), t[:, :, :2])


def test_make_eigenmodes_refuses_before_the_gpu(zd, capfd):
    """odd n, n < 4, n > 512: non-zero, a message, nothing written — checked here without a GPU, because the refusal comes first"""
    L = zd.load_library()
    buf = np.full(64, -7.0)
    for n in (7, 2, 0, -4, 514, 1024):
        assert L.zd_make_eigenmodes(n, buf.ctypes.data) != 0
        assert "even number of points per side in [4, 512]" in capfd.readouterr().err
        assert np.all(buf == -7.0)
        with pytest.raises(ValueError):
            zd.make_eigenmodes(n)
    assert L.zd_make_eigenmodes(8, None) != 0
