"""GPU: band power of the realised modes (zd_measure_power / zd_plan_measure_power, csrc/zd_kernels_pk.hip) against the oracle's
mode cubes, bin for bin (tests/power_ref.py is the numpy restatement of the definition), against closed forms at full size and
against the production run's own statistic."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import power_ref as pr
from conftest import ROOT, WMAP

pytestmark = pytest.mark.gpu
BOX = 720.0
EXE = os.path.join(ROOT, "zeldovich_plt_amd", "csrc", "build", "zeldovich")


@pytest.fixture(scope="module")
def zd():
    import zeldovich_plt_amd.api as api
    return api


def _spectra(zd, oracle, kind, fix=0):
    if kind == "plaw":
        return (zd.PowerSpectrum.from_powerlaw(-1.5, BOX, fix_to_mean=fix), oracle.pk_from_powerlaw(-1.5, BOX, fix_to_mean=fix))
    return zd.PowerSpectrum.from_file(WMAP, BOX, fix_to_mean=fix), oracle.pk_from_file(WMAP, BOX, fix_to_mean=fix)


def _report(name, got, ref):
    for key in ("sum_k", "sum_dens", "sum_input"):
        print("%s: worst relative difference of %s over the bins = %.3g" % (name, key, pr.worst(got[key], ref[key])))


DENSITY_CASES = [
    (32, "file", dict()), (64, "file", dict()), (128, "file", dict()),
    (64, "file", dict(k_cutoff=2.0)), (128, "file", dict(k_cutoff=2.0)),
    (64, "file", dict(corner_modes=1)),                       # CornerModes at k_cutoff = 1: the cube's corners stay alive
    (64, "plaw", dict()), (32, "plaw", dict(k_cutoff=2.0)),
    (64, "file", dict(fix=1)), (128, "plaw", dict(fix=1)),    # fixed amplitudes
    (64, "file", dict(qonemode=1, one_mode=(3, 5, -7))), (32, "file", dict(qonemode=1, one_mode=(2, 0, 4))),
    (96, "file", dict()), (96, "file", dict(k_cutoff=2.0)),   # composite family
    (100, "file", dict()), (100, "plaw", dict(w=3)),          # convolution family
    (64, "file", dict(w=2)), (128, "file", dict(w=7)),
]


@pytest.mark.parametrize("n,kind,kw", DENSITY_CASES)
def test_density_sums_against_the_oracle_cube(zd, oracle, n, kind, kw):
    """count exact; sum_dens, sum_input to 1e-12 of the bin's value (the per-mode bound on D(k) is 1e-13, this is a sum of its
    squares); sum_k to 1e-14"""
    kw = dict(kw)
    w, fix = kw.pop("w", 1), kw.pop("fix", 0)
    ps, opk = _spectra(zd, oracle, kind, fix)
    okw = dict(kw)
    if "corner_modes" in okw:
        okw["CornerModes"] = okw.pop("corner_modes")
    D = oracle.mode_cube(oracle.make_params(n, qdensity=2, **okw), opk)[0]
    ref = pr.reference_sums(oracle, opk, n, BOX, D, w)
    got = zd.measure_power(zd.make_params(n, **kw), ps, bin_width=w)
    _report("PPD %d %s %r w=%d" % (n, kind, kw, w), got, ref)
    assert len(got["count"]) == pr.nbins(n, w)
    assert np.array_equal(got["count"], ref["count"])
    assert ref["count"].sum() > 0
    assert pr.close(got["sum_dens"], ref["sum_dens"], 1e-12)
    assert pr.close(got["sum_input"], ref["sum_input"], 1e-12)
    assert pr.close(got["sum_k"], ref["sum_k"], 1e-14)
    if fix:
        assert pr.close(got["sum_dens"], np.asarray(got["sum_input"], dtype=np.longdouble), 1e-13)
    # derived columns
    live = got["count"] > 0
    assert np.array_equal(got["nmodes"], got["count"])
    assert np.allclose(got["k_mean"][live], got["sum_k"][live] / got["count"][live], rtol=0, atol=0)
    assert np.allclose(got["P_measured / P_input"][live], got["sum_dens"][live] / got["sum_input"][live], rtol=0, atol=0)
    # ZA: v = vnorm q with vnorm = (sqrt(1 + 24 f_cluster) - 1) / 4 = 1 at f_cluster = 1, q_j = i k_j fundamental D / k^2
    assert pr.close(got["sum_vel"], np.asarray(got["sum_disp"], dtype=np.longdouble), 1e-14)


@pytest.mark.parametrize("kind", ["file", "plaw"])
@pytest.mark.parametrize("eig_ppd", [16, 24, 64])  # 16, 24: trilinear blends (24: no common cell edges with the grid of 64); 64: exact stride
@pytest.mark.parametrize("rescale", [0, 1])
def test_plt_displacement_and_velocity_power(zd, oracle, kind, eig_ppd, rescale):
    """PLT at PPD = 64: sum_disp / sum_vel against the Hermitian and anti-Hermitian parts of the oracle's four packed arrays
    (D + i qx | qy + i qz | vx-array | vy + i vz), 1e-12 of the bin's value"""
    n = 64
    ps, opk = _spectra(zd, oracle, kind)
    eig = oracle.synthetic_eigenmodes(eig_ppd)
    kw = dict(qPLT=1, qPLTrescale=rescale, PLT_target_z=5.0, f_cluster=0.9)
    cube = oracle.mode_cube(oracle.make_params(n, **kw), opk, eig=eig, eig_ppd=eig_ppd)
    assert cube.shape[0] == 4
    parts = [pr.hermitian_parts(cube[a]) for a in range(4)]
    D = parts[0][0]
    mask = pr.alive_mask(oracle.mode_cube(oracle.make_params(n, qdensity=2), opk)[0])
    nb, bins = pr.nbins(n, 1), pr.bin_cube(n, 1)
    a2 = lambda f: f.real.astype(np.longdouble) ** 2 + f.imag.astype(np.longdouble) ** 2
    disp = pr.binsum(a2(parts[0][1]) + a2(parts[1][0]) + a2(parts[1][1]), bins, mask, nb)
    vel = pr.binsum(a2(parts[2][0]) + a2(parts[2][1]) + a2(parts[3][0]) + a2(parts[3][1]), bins, mask, nb)
    dens = pr.binsum(a2(D), bins, mask, nb)
    got = zd.measure_power(zd.make_params(n, **kw), ps, eig=eig)
    for name, g, r in (("sum_dens", got["sum_dens"], dens), ("sum_disp", got["sum_disp"], disp), ("sum_vel", got["sum_vel"], vel)):
        print("PLT eig %d rescale %d %s: worst relative difference of %s = %.3g" % (eig_ppd, rescale, kind, name, pr.worst(g, r)))
    assert np.array_equal(got["count"], np.bincount(bins[mask], minlength=nb))
    assert pr.close(got["sum_dens"], dens, 1e-12)
    assert pr.close(got["sum_disp"], disp, 1e-12)
    assert pr.close(got["sum_vel"], vel, 1e-12)
    assert disp.sum() > 0 and vel.sum() > 0 and abs(float(vel.sum() / disp.sum()) - 1) > 1e-3  # the velocity is its own field


def test_za_velocity_is_vnorm_times_displacement(zd, oracle):
    """ZA at f_cluster != 1: sum_vel = vnorm^2 sum_disp, and sum_disp against the oracle's arrays D + i qx | qy + i qz"""
    n, fc = 64, 0.8
    ps, opk = _spectra(zd, oracle, "file")
    cube = oracle.mode_cube(oracle.make_params(n, f_cluster=fc), opk)
    assert cube.shape[0] == 2
    parts = [pr.hermitian_parts(cube[a]) for a in range(2)]
    mask = pr.alive_mask(parts[0][0])
    nb, bins = pr.nbins(n, 1), pr.bin_cube(n, 1)
    a2 = lambda f: f.real.astype(np.longdouble) ** 2 + f.imag.astype(np.longdouble) ** 2
    disp = pr.binsum(a2(parts[0][1]) + a2(parts[1][0]) + a2(parts[1][1]), bins, mask, nb)
    got = zd.measure_power(zd.make_params(n, f_cluster=fc), ps)
    vnorm = (np.sqrt(1 + 24 * fc) - 1) / 4
    assert pr.close(got["sum_disp"], disp, 1e-12)
    assert pr.close(got["sum_vel"], np.asarray(got["sum_disp"], dtype=np.longdouble) * np.longdouble(vnorm) ** 2, 1e-14)


def test_fnl_density_power(zd, oracle):
    """ZD_f_NL = 2e4 at PPD = 64: D = PhiK M of the plan's own PhiK against the numpy forward transform of the oracle's density
    planes; 1e-10 of the largest bin (two FFT round trips lie between the two sides: the project's field tolerance)"""
    n, fnl, ns, om = 64, 2.0e4, 0.96, 0.31
    ps, opk = _spectra(zd, oracle, "file")
    oracle.lib().zdo_pk_set_primordial(C.byref(opk), ns)
    out = oracle.run(oracle.make_params(n, numblock=2, qdensity=2, f_NL=fnl, n_s=ns, Omega_M=om), opk, want_planes=True)
    dens = out["planes"][:, 0].real.transpose(1, 0, 2)  # [y][z][x]
    D = np.fft.fftn(dens) / n ** 3                      # [ky][kz][kx]
    mask = pr.alive_mask(oracle.mode_cube(oracle.make_params(n, qdensity=2), opk)[0])
    nb, bins = pr.nbins(n, 1), pr.bin_cube(n, 1)
    want = pr.binsum(D.real.astype(np.longdouble) ** 2 + D.imag.astype(np.longdouble) ** 2, bins, mask, nb)
    lin = pr.reference_sums(oracle, opk, n, BOX, oracle.mode_cube(oracle.make_params(n, qdensity=2), opk)[0])
    got = zd.measure_power(zd.make_params(n, f_NL=fnl, n_s=ns, Omega_M=om), ps)
    err = np.abs(np.asarray(got["sum_dens"], dtype=np.longdouble) - want).max() / want.max()
    print("f_NL: largest difference of sum_dens / largest bin = %.3g" % float(err))
    assert np.array_equal(got["count"], lin["count"])
    assert err <= 1e-10
    assert np.abs(want - lin["sum_dens"]).max() > 1e-6 * want.max()  # the non-Gaussian term is really there
    assert pr.close(got["sum_input"], lin["sum_input"], 1e-12)


def test_full_size_fixed_amplitudes_are_exact(zd):
    """PPD = 2048 with ZD_qPk_fix_to_mean: |D|^2 = P(k) mode by mode, so sum_dens = sum_input per bin to 1e-13"""
    n = 2048
    ps = zd.PowerSpectrum.from_file(WMAP, BOX, fix_to_mean=1)
    got = zd.measure_power(zd.make_params(n, icformat="RVZel"), ps)
    live = got["count"] > 0
    rel = np.abs(got["sum_dens"][live] / got["sum_input"][live] - 1)
    print("PPD 2048 fixed amplitudes: worst |sum_dens / sum_input - 1| = %.3g over %d bins" % (rel.max(), live.sum()))
    assert live.sum() > 1000 and rel.max() <= 1e-13
    # every live mode of the cube is counted: the sphere |k| < N/2 minus the planes |k_i| = N/2 and the origin
    k = pr.ksigned(n)
    below = np.cumsum(np.bincount((k[:, None] ** 2 + k[None, :] ** 2).ravel()))  # (kx, ky) pairs with kx^2 + ky^2 <= index
    lim = (n // 2) ** 2 - k * k - 1                                               # ... needed: kx^2 + ky^2 <= lim
    total = int(below[lim[lim >= 0]].sum())
    assert got["count"].sum() == total - 1


@pytest.mark.parametrize("n", [1024, 4096])
def test_parseval_against_the_production_run(zd, n):
    """ZA, default store: N^3 sum_b sum_dens = density_variance of the production run to 1e-10 (the bound on that statistic)"""
    ps = zd.PowerSpectrum.from_file(WMAP, BOX)
    p = zd.make_params(n, icformat="RVZel", numblock=64)
    var = zd.generate(p, ps, collect=False)["density_variance"]
    got = zd.measure_power(zd.make_params(n, icformat="RVZel", numblock=64), ps)
    total = float(np.sum(got["sum_dens"].astype(np.longdouble))) * float(n) ** 3
    print("PPD %d: N^3 sum |D|^2 = %.17g, density_variance = %.17g, relative difference %.3g" % (n, total, var, abs(total - var) / var))
    assert abs(total - var) <= 1e-10 * var


def test_oversampled_grid_measures_the_coarse_grid(zd):
    """PPD = 4096 with ZD_k_cutoff = 2 realises the modes of PPD = 2048 with ZD_k_cutoff = 1: bin for bin at w = 1, counts exact,
    sums to 1e-12"""
    ps = zd.PowerSpectrum.from_file(WMAP, BOX)
    fine = zd.measure_power(zd.make_params(4096, icformat="RVZel", numblock=64, k_cutoff=2.0), ps)
    coarse = zd.measure_power(zd.make_params(2048, icformat="RVZel", numblock=64), ps)
    nb = len(coarse["count"])
    assert np.array_equal(fine["count"][:nb], coarse["count"]) and fine["count"][nb:].sum() == 0 and coarse["count"].sum() > 0
    for key in zd.POWER_SUMS:
        a, b = fine[key][:nb].astype(np.longdouble), coarse[key].astype(np.longdouble)
        print("oversampling: worst relative difference of %s = %.3g" % (key, pr.worst(a, b)))
        assert pr.close(a, b, 1e-12), key


@pytest.mark.parametrize("plt", [False, True])
@pytest.mark.parametrize("nranks", [2, 4])
def test_rank_sums_add_up(zd, oracle, plt, nranks):
    """plans of 2 and 4 ranks sharing the GPU: their sums add to the single-rank result; counts exact, sums to 1e-13"""
    n = 256
    ps = zd.PowerSpectrum.from_file(WMAP, BOX)
    eig = oracle.synthetic_eigenmodes(32) if plt else None
    kw = dict(qPLT=1, qPLTrescale=1, PLT_target_z=5.0) if plt else dict(stream_factor=2)
    one = zd.Plan(zd.make_params(n, **kw), ps, eig=eig)
    whole = one.measure_power()
    one.close()
    acc = None
    for r in range(nranks):
        pl = zd.Plan(zd.make_params(n, **kw), ps, eig=eig, rank=r, nranks=nranks)
        part = pl.measure_power()
        pl.close()
        assert part["count"].sum() > 0
        if acc is None:
            acc = {k: part[k].astype(np.longdouble) if k != "count" else part[k].copy() for k in ("count",) + zd.POWER_SUMS}
        else:
            for k in ("count",) + zd.POWER_SUMS:
                acc[k] = acc[k] + part[k]
    assert np.array_equal(acc["count"], whole["count"])
    for k in zd.POWER_SUMS:
        assert pr.close(whole[k], acc[k], 1e-13), k


def test_refusals(zd, capfd):
    """live Nyquist planes (CornerModes with k_cutoff = 2) and ZD_Version = 1: non-zero return, a message, no crash"""
    ps = zd.PowerSpectrum.from_file(WMAP, BOX)
    with pytest.raises(RuntimeError):
        zd.measure_power(zd.make_params(64, corner_modes=1, k_cutoff=2.0), ps)
    assert "Nyquist" in capfd.readouterr().err
    with pytest.raises(RuntimeError):
        zd.measure_power(zd.make_params(64, version=1), ps)
    assert "ZD_Version = 1" in capfd.readouterr().err
    with pytest.raises(ValueError):
        zd.measure_power(zd.make_params(64), ps, bin_width=0)
    # too few bins: refused by the library, nothing written
    L = zd.load_library()
    p = zd.make_params(64)
    arrs = [np.zeros(4, dtype=np.int64)] + [np.zeros(4) for _ in range(5)]
    assert L.zd_measure_power(C.byref(p), C.byref(ps.pk), None, 0, 1, 4, *[a.ctypes.data for a in arrs]) != 0
    assert all(not a.any() for a in arrs)
    # ... and the library still measures afterwards
    assert zd.measure_power(zd.make_params(64), ps)["count"].sum() > 0


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
"""


def test_cli_writes_the_measured_power_table(zd, tmp_path):
    """ZD_Pk_measured_filename: a table whose columns match measure_power; without the key no table, and the same ic_* bytes"""
    outs = []
    table = tmp_path / "pk_measured.txt"
    for i, extra in enumerate(("", 'ZD_Pk_measured_filename = "%s"\n' % table)):
        out = tmp_path / ("ic%d" % i)
        out.mkdir()
        par = tmp_path / ("t%d.par" % i)
        par.write_text(PAR % dict(out=out, pk=WMAP) + extra)
        r = subprocess.run([EXE, str(par)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        if not extra:
            assert not table.exists() and "band power" not in r.stderr
        else:
            assert "worst |P_measured / P_input - 1| sqrt(count)" in r.stderr
            worst_line = float(r.stderr.split("sqrt(count) over the bins is")[1].split()[0])
        outs.append(out)
    files = sorted(f.name for f in outs[0].iterdir())
    assert files and files == sorted(f.name for f in outs[1].iterdir())
    for f in files:
        assert (outs[0] / f).read_bytes() == (outs[1] / f).read_bytes(), f
    lines = table.read_text().splitlines()
    assert lines[0] == "# k_mean count P_measured P_input disp_power vel_power"
    tab = np.array([[float(v) for v in ln.split()] for ln in lines[1:]])
    got = zd.measure_power(zd.make_params(64), zd.PowerSpectrum.from_file(WMAP, BOX))
    live = got["count"] > 0
    n = got["count"][live].astype(np.float64)
    assert tab.shape == (live.sum(), 6)
    assert np.array_equal(tab[:, 1], n)
    for col, key in ((0, "sum_k"), (2, "sum_dens"), (3, "sum_input"), (4, "sum_disp"), (5, "sum_vel")):
        assert np.allclose(tab[:, col], got[key][live] / n, rtol=1e-13, atol=0), key
    ratio = got["sum_dens"][live] / got["sum_input"][live]
    assert abs(worst_line - np.max(np.abs(ratio - 1) * np.sqrt(n))) <= 1e-5 * worst_line
    assert 0.5 < worst_line < 8.0  # Gaussian draws: |ratio - 1| sqrt(count) is of order one in every bin
