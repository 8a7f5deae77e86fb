"""GPU: second order (2LPT) on a caller-supplied field (generate_field(order=2), Plan.from_field(order=2), ZD_Field_order; definition in
zeldovich_plt_amd/csrc/zd_kernels_lpt2_field.hip).

The yardstick is tests/field_lpt2_ref.py: field_ref.displace for the first order of the field, lpt2_ref.second_order of that displacement
for the second (tests/test_field_lpt2.py holds the two alive masks to each other and the second-order term of these fields to >= 5 % of
the first).  The second-order part of a run is compared on its own, as tests/test_gpu_lpt2.py does — (d2 - d1) against gamma psi2_ref,
(v2 - alpha d1) against f2 gamma psi2_ref, to 1e-10 of max|psi2_ref|, the project's parity bound applied to the small term — where d1 is
the order = 1 run of the same field, itself held to numpy at 1e-10 of max|q|.  Every test prints its figures before it asserts."""
import os
import re
import subprocess

import numpy as np
import pytest

import field_lpt2_ref
import field_ref
from conftest import ROOT, WMAP

pytestmark = pytest.mark.gpu

BOX = 720.0
TOL = 1e-10
SIGMA = 0.42  # the seeded second-order tests' (tests/test_gpu_lpt2.py)
XYZ = [2, 1, 0]
EXE = os.path.join(ROOT, "zeldovich_plt_amd", "csrc", "build", "zeldovich")


@pytest.fixture(scope="module")
def zd():
    import zeldovich_plt_amd.api as api
    return api


@pytest.fixture(scope="module")
def ps(zd):
    return zd.PowerSpectrum.from_file(WMAP, BOX)


_NOISE, _REF, _RUN1 = {}, {}, {}


def _noise(n, amp=1.0):
    """amp * default_rng(1).standard_normal((n, n, n)) (shared, read-only)"""
    if (n, amp) not in _NOISE:
        a = amp * np.random.default_rng(1).standard_normal((n, n, n))
        a.setflags(write=False)
        _NOISE[(n, amp)] = a
    return _NOISE[(n, amp)]


def _reference(zd, n, k_cutoff=1.0, amp=1.0, f_cluster=1.0):
    """(q, psi2 at gamma = 1) of numpy for the density amp * noise, once per configuration"""
    key = (n, k_cutoff, amp, f_cluster)
    if key not in _REF:
        q, psi2 = field_lpt2_ref.first_and_unit_second(_noise(n, amp), zd.make_params(n, boxsize=BOX, k_cutoff=k_cutoff, f_cluster=f_cluster), BOX)
        q.setflags(write=False)
        psi2.setflags(write=False)
        _REF[key] = (q, psi2)
    return _REF[key]


def _first_order(zd, ps, n, k_cutoff=1.0, amp=1.0, f_cluster=1.0):
    """the order = 1 records of the same field, held to numpy, once per configuration"""
    key = (n, k_cutoff, amp, f_cluster)
    if key not in _RUN1:
        q, _psi2 = _reference(zd, n, k_cutoff, amp, f_cluster)
        rec = zd.generate_field(zd.make_params(n, boxsize=BOX, k_cutoff=k_cutoff, f_cluster=f_cluster), ps, _noise(n, amp), order=1)["records"]
        e1 = np.abs(rec["d"] - q).max() / np.abs(q).max()
        print("PPD", n, "k_cutoff", k_cutoff, "order 1 against numpy:", e1)
        assert e1 <= TOL
        _RUN1[key] = rec
    return _RUN1[key]


def _check_second_order(got2, got1, psi2_ref, alpha, f2, label):
    """the second-order part on its own, displacement and velocity; prints the figures before it asserts"""
    scale = np.abs(psi2_ref).max()
    ed = np.abs((got2["d"] - got1["d"]) - psi2_ref).max() / scale
    ev = np.abs((got2["v"] - alpha * got1["d"]) - f2 * psi2_ref).max() / scale
    print(label, "max|psi2_ref| =", scale, "max|psi2_ref| / max|q| =", scale / np.abs(got1["d"]).max(), "displacement error", ed, "velocity error", ev)
    assert np.array_equal(got2["ijk"], got1["ijk"]) and np.array_equal(got2["pad"], got1["pad"])
    assert ed <= TOL and ev <= TOL, (label, ed, ev)


# ---- 1. every record against numpy -------------------------------------------------------------------------------------------
CASES = [(32, 1.0, 0), (64, 1.0, 0), (128, 1.0, 0), (64, 2.0, 0), (128, 2.0, 0), (64, 1.0, 2), (64, 1.0, 4), (128, 1.0, 4)]


@pytest.mark.parametrize("n,k_cutoff,R", CASES, ids=["%d-kc%g-R%d" % c for c in CASES])
def test_records_against_numpy(zd, ps, n, k_cutoff, R):
    """(64 at stream factor 4: z lines of 16 points, the shortest the final pass runs; k_cutoff = 2 on 2 x the field)"""
    amp = 2.0 if k_cutoff == 2.0 else 1.0
    q, psi2_unit = _reference(zd, n, k_cutoff, amp)
    psi2_ref = (3.0 / 7.0) * psi2_unit
    ratio = np.abs(psi2_ref).max() / np.abs(q).max()
    print("PPD", n, "k_cutoff", k_cutoff, "reference max|psi2| / max|psi1| =", ratio)
    assert ratio >= 0.05
    one = _first_order(zd, ps, n, k_cutoff, amp)
    got = zd.generate_field(zd.make_params(n, boxsize=BOX, k_cutoff=k_cutoff, stream_factor=R), ps, _noise(n, amp), order=2)
    assert got["stream_factor"] == max(R, 1) and sorted(got["planes_seen"]) == list(range(n))
    _check_second_order(got["records"], one, psi2_ref, 1.0, 2.0, "PPD %d k_cutoff %g R %d" % (n, k_cutoff, R))
    if R > 1:  # the same field whatever the stream factor
        r1 = zd.generate_field(zd.make_params(n, boxsize=BOX, k_cutoff=k_cutoff, stream_factor=1), ps, _noise(n, amp), order=2)["records"]
        for f in ("d", "v"):
            e = np.abs(got["records"][f] - r1[f]).max() / np.abs(r1[f]).max()
            print("stream factor", R, "against 1:", f, e)
            assert e <= 1e-12
        assert np.array_equal(got["records"]["ijk"], r1["ijk"])


def test_white_noise_against_numpy(zd, ps):
    """kind = "white": the second order of the coloured density (field_ref.white_to_density); ZD_Pk_sigma raised as in the seeded tests"""
    n = 64
    pw = zd.PowerSpectrum.from_file(WMAP, BOX, Pk_sigma=SIGMA)
    p = zd.make_params(n, boxsize=BOX)
    delta = field_ref.white_to_density(_noise(n), pw, p)
    q, psi2_unit = field_lpt2_ref.first_and_unit_second(delta, p, BOX)
    psi2_ref = (3.0 / 7.0) * psi2_unit
    ratio = np.abs(psi2_ref).max() / np.abs(q).max()
    print("white noise at PPD 64: reference max|psi2| / max|psi1| =", ratio)
    assert ratio >= 0.05
    one = zd.generate_field(p, pw, _noise(n), kind="white", order=1)["records"]
    e1 = np.abs(one["d"] - q).max() / np.abs(q).max()
    print("order 1 against numpy:", e1)
    assert e1 <= TOL
    got = zd.generate_field(p, pw, _noise(n), kind="white", order=2)["records"]
    _check_second_order(got, one, psi2_ref, 1.0, 2.0, "PPD 64 white")


# ---- 2. seeds and fields meet --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 256])
def test_the_density_of_a_seeded_run_returns_its_second_order_records(zd, n):
    pw = zd.PowerSpectrum.from_file(WMAP, BOX, Pk_sigma=SIGMA)
    za = zd.generate(zd.make_params(n, boxsize=BOX), pw)["records"]
    ref = zd.generate(zd.make_params(n, boxsize=BOX, q2LPT=1), pw)["records"]
    delta = field_ref.delta_from_za(za, BOX)
    got = zd.generate_field(zd.make_params(n, boxsize=BOX, seed=999), pw, delta, order=2)["records"]  # (ZD_Seed is ignored)
    one = zd.generate_field(zd.make_params(n, boxsize=BOX), pw, delta, order=1)["records"]
    scale, s2 = np.abs(ref["d"]).max(), np.abs(ref["d"] - za["d"]).max()
    ed, ev = np.abs(got["d"] - ref["d"]).max() / scale, np.abs(got["v"] - ref["v"]).max() / scale
    e2 = np.abs((got["d"] - one["d"]) - (ref["d"] - za["d"])).max() / s2
    print("PPD", n, "max|q| =", scale, "max|d2 - d1| / max|q| =", s2 / scale, "displacement error", ed, "velocity error", ev, "second-order part", e2)
    assert s2 >= 0.05 * scale and np.array_equal(got["ijk"], ref["ijk"])
    assert ed <= TOL and ev <= TOL and e2 <= TOL


# ---- 3. coefficients -----------------------------------------------------------------------------------------------------------
def test_given_coefficients_scale_the_two_parts(zd, ps):
    n, fcl = 64, 0.9
    q, psi2_unit = _reference(zd, n, 1.0, 1.0, fcl)
    one = _first_order(zd, ps, n, 1.0, 1.0, fcl)
    alpha, gamma0, f20 = field_lpt2_ref.coefficients(zd.make_params(n, boxsize=BOX, f_cluster=fcl))
    assert np.abs(one["v"] - alpha * one["d"]).max() <= 1e-15 * np.abs(one["d"]).max()
    got = zd.generate_field(zd.make_params(n, boxsize=BOX, f_cluster=fcl, lpt2_ratio=-0.5, lpt2_f2=1.7), ps, _noise(n), order=2)["records"]
    _check_second_order(got, one, 0.5 * psi2_unit, alpha, 1.7, "given coefficients")
    got = zd.generate_field(zd.make_params(n, boxsize=BOX, f_cluster=fcl), ps, _noise(n), order=2)["records"]
    _check_second_order(got, one, gamma0 * psi2_unit, alpha, f20, "defaults at f_cluster 0.9")


# ---- 4. one plane wave: S = 0 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 1024])
def test_one_plane_wave_has_no_second_order(zd, ps, n):
    """one plane of the run through ZD_qoneslab; the field is built on the device (1024: 8.6 GB of float64)"""
    import torch
    field = field_ref.plane_waves(n, [((3, 5, -2), 1.0, 0.4)], BOX, [(0, 0, 0)], xp=torch, device="cuda")[0]
    planes = {}
    for order in (1, 2):
        got = {}

        def take(z, plane):
            got[z] = plane.copy()

        R = 2 if n == 64 else 4  # (an order = 1 run takes no z lines under 32 points)
        st = zd.generate_field(zd.make_params(n, boxsize=BOX, qoneslab=7, stream_factor=R), ps, field, order=order, on_plane=take)
        assert list(got) == [7] and st["planes"] == 1
        planes[order] = got[7]
    scale = np.abs(planes[1]["d"]).max()
    ed, ev = np.abs(planes[2]["d"] - planes[1]["d"]).max() / scale, np.abs(planes[2]["v"] - planes[1]["v"]).max() / scale
    print("PPD", n, "one wave: max|q| =", scale, "second-order part of d", ed, "of v", ev)
    assert scale > 0 and np.array_equal(planes[2]["ijk"], planes[1]["ijk"])
    assert ed <= 1e-12 and ev <= 1e-12


def _plan_planes(zd, plan, n, zs):
    """the record planes zs of a plan through the stage calls: {z: records[y, x]}"""
    import torch
    dt = zd.RECORD_DTYPES["RVdoubleZel"]
    assert plan.record_size == dt.itemsize and plan.plane_step == 1
    store = torch.empty(plan.exchange_bytes, dtype=torch.uint8, device="cuda")
    rec = torch.empty(n * n * dt.itemsize, dtype=torch.uint8, device="cuda")
    where = {plan.plane_z(r, lp): (r, lp) for r in range(plan.passes) for lp in range(plan.local_planes)}
    out = {}
    for r in sorted({where[z][0] for z in zs}):
        plan.stage_z(r, store.data_ptr())
        plan.stage_y(store.data_ptr())
        for z in zs:
            if where[z][0] == r:
                plan.stage_x(r, store.data_ptr(), where[z][1], 1, rec.data_ptr())
                torch.cuda.synchronize()
                out[z] = rec.cpu().numpy().view(dt).reshape(n, n).copy()
    return out


# ---- 5. the four ICFormats -----------------------------------------------------------------------------------------------------
def test_record_formats(zd, ps):
    n = 32
    ref = zd.generate_field(zd.make_params(n, boxsize=BOX), ps, _noise(n), order=2)["records"]
    for fmt in ("RVZel", "Zeldovich", "ZelSimple"):
        got = zd.generate_field(zd.make_params(n, boxsize=BOX, icformat=fmt), ps, _noise(n), order=2)["records"]
        if "ijk" in got.dtype.names:
            assert np.array_equal(got["ijk"], ref["ijk"])
        for f in ("d", "v"):
            if f in got.dtype.names:  # (cast as the parity tests cast: 1e-6 for the float32 members)
                tol = TOL if got[f].dtype == np.float64 else 1e-6
                err = np.abs(got[f] - ref[f]).max() / np.abs(ref[f]).max()
                print(fmt, f, "error", err)
                assert err <= tol, (fmt, f, err)


# ---- 6. input forms ------------------------------------------------------------------------------------------------------------
def test_input_forms_give_identical_bits(zd, ps):
    import torch
    n = 64
    a64 = _noise(n).astype(np.float32).astype(np.float64)  # float64 values that float32 holds exactly
    a32 = a64.astype(np.float32)
    p = zd.make_params(n, boxsize=BOX)
    forms = {"host float64": a64, "host float32": a32, "device float64": torch.from_numpy(a64).cuda(), "device float32": torch.from_numpy(a32).cuda()}
    base = zd.generate_field(p, ps, a64, order=2)["records"].tobytes()
    assert base != zd.generate_field(p, ps, a64, order=1)["records"].tobytes()
    for name, f in forms.items():
        assert zd.generate_field(p, ps, f, order=2)["records"].tobytes() == base, name


# ---- 7. the plan ---------------------------------------------------------------------------------------------------------------
def test_the_plan_is_a_second_order_plan(zd, ps, capfd):
    import torch
    n = 64
    p = zd.make_params(n, boxsize=BOX, stream_factor=2)
    rec = zd.generate_field(p, ps, _noise(n), order=2)["records"]
    q, psi2_unit = _reference(zd, n)
    plan = zd.Plan.from_field(p, ps, _noise(n), order=2)
    try:
        assert plan.narray == 4 and plan.store_mode == "reference" and plan.R == 2
        dt = zd.RECORD_DTYPES["RVdoubleZel"]
        store = torch.empty(plan.exchange_bytes, dtype=torch.uint8, device="cuda")
        chunk = torch.empty(plan.local_planes * n * n * dt.itemsize, dtype=torch.uint8, device="cuda")

        def run():
            out = {}

            def consume(pass_, first, cnt, ptr, st):
                torch.cuda.synchronize()
                host = chunk[:cnt * n * n * dt.itemsize].cpu().numpy().view(dt).reshape(cnt, n, n)
                for i in range(cnt):
                    out[plan.plane_z(pass_, first + i)] = host[i].copy()
                return 0

            plan.run_passes(0, 1, store.data_ptr(), None, chunk.data_ptr(), plan.local_planes, consume=consume)
            torch.cuda.synchronize()
            return np.stack([out[z] for z in range(n)])

        a, b = run(), run()
        assert a.tobytes() == b.tobytes() == rec.tobytes()
        # the orders at sites: their sum is the delivered record, order 2 is numpy's gamma psi2
        sites = np.random.default_rng(5).integers(0, n, (8, 3))
        at = (sites[:, 0], sites[:, 1], sites[:, 2])
        got = plan.lpt_direct_sum(sites)
        tot, scale, s2 = got.sum(axis=1), np.abs(rec["d"]).max(), (3.0 / 7.0) * np.abs(psi2_unit).max()
        ed = np.abs(tot[:, 0:3][:, XYZ] - rec["d"][at]).max() / scale
        ev = np.abs(tot[:, 3:6][:, XYZ] - rec["v"][at]).max() / scale
        e2 = np.abs(got[:, 1, 0:3][:, XYZ] - (3.0 / 7.0) * psi2_unit[at]).max() / s2
        e1 = np.abs(got[:, 0, 0:3][:, XYZ] - q[at]).max() / np.abs(q).max()
        print("lpt_direct_sum at PPD 64: sum of orders d", ed, "v", ev, "order 1 against numpy", e1, "order 2 against numpy", e2)
        assert ed <= TOL and ev <= TOL and e1 <= TOL and e2 <= TOL and np.all(got[:, 2] == 0.0)
        # band power: numpy's binning of the masked |D|^2 over all N^3 wavevectors
        D = np.fft.fftn(_noise(n)) / n ** 3 * field_ref.alive_mask(p)
        k = field_ref.wavenumbers(n)
        kz, ky, kx = np.meshgrid(k, k, k, indexing="ij")
        shell = np.floor(np.sqrt((kx * kx + ky * ky + kz * kz).astype(np.float64))).astype(np.int64)
        pw = plan.lpt_power(1)
        nb = len(pw["sum_dens"])
        want = np.bincount(shell.ravel(), weights=(np.abs(D) ** 2).ravel(), minlength=nb)[:nb]
        live = want > 0
        e3 = np.abs(pw["sum_dens"][live] / want[live] - 1.0).max()
        print("lpt_power: worst relative shell error of sum_dens =", e3, "shells", int(live.sum()), "sum_disp2 / sum_disp1 =", pw["sum_disp2"].sum() / pw["sum_disp1"].sum())
        assert live.sum() > 20 and e3 <= 1e-12 and np.all(pw["sum_dens"][~live] == 0.0) and pw["sum_disp2"].sum() > 0
        # ... and what every second-order plan refuses
        capfd.readouterr()
        with pytest.raises(RuntimeError):
            plan.measure_power(1)
        assert "ZD_q2LPT" in capfd.readouterr().err
        with pytest.raises(RuntimeError):
            plan.direct_sum(sites)
        assert "ZD_q2LPT" in capfd.readouterr().err
    finally:
        plan.close()


@pytest.mark.parametrize("n", [128, 512])
def test_the_orders_of_the_plan_sum_to_its_records(zd, ps, n):
    """a torch field on the device at stream factor 2; eight sites on two planes, one of each z residue (512: the second workgroup
    along x of the sums); the delivered planes come from the stage calls"""
    import torch
    gen = torch.Generator(device="cuda")
    gen.manual_seed(n)
    field = torch.randn((n, n, n), dtype=torch.float64, device="cuda", generator=gen)
    rng = np.random.default_rng(n)
    sites = np.column_stack([np.repeat([17, 18], 4), rng.integers(0, n, (8, 2))]).astype(np.int64)
    sites[0, 2], sites[1, 2], sites[4, 2] = 0, n - 1, n // 2
    p = zd.make_params(n, boxsize=BOX, stream_factor=2)
    planes = {}
    for order in (1, 2):
        plan = zd.Plan.from_field(p, ps, field, order=order)
        try:
            assert plan.R == 2
            planes[order] = _plan_planes(zd, plan, n, [17, 18])
            if order == 2:
                got = plan.lpt_direct_sum(sites)
        finally:
            plan.close()
    scale = max(np.abs(pl["d"]).max() for pl in planes[2].values())
    tot, s2 = got.sum(axis=1), np.abs(got[:, 1, 0:3]).max()
    ed = ev = e2 = 0.0
    for i, (z, y, x) in enumerate(sites):
        r2, r1 = planes[2][int(z)][y, x], planes[1][int(z)][y, x]
        ed = max(ed, np.abs(tot[i, 0:3][XYZ] - r2["d"]).max() / scale)
        ev = max(ev, np.abs(tot[i, 3:6][XYZ] - r2["v"]).max() / scale)
        e2 = max(e2, np.abs(got[i, 1, 0:3][XYZ] - (r2["d"] - r1["d"])).max() / s2)
    print("PPD", n, "max|q| on the planes =", scale, "max|order 2| / max|q| =", s2 / scale, "sum of orders: d", ed, "v", ev, "order 2 alone", e2)
    assert s2 > 0 and ed <= TOL and ev <= TOL and e2 <= TOL


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------
def _one_field_line(err, word):
    lines = [ln for ln in err.splitlines() if ln.startswith("zeldovich_hip: ZD_Field")]
    assert len(lines) == 1 and word in lines[0], (word, err)
    return lines[0]


REFUSED = [  # (order, make_params arguments, the word the line names)
    (3, {}, "order = 3"),
    (2, dict(q2LPT=1), "ZD_q2LPT"),
    (2, dict(qPLT=1), "ZD_qPLT"),
    (2, dict(qdensity=1), "ZD_qdensity"),
    (2, dict(f_NL=50.0), "ZD_f_NL"),
    (2, dict(ngpu=2), "ZD_NumGPU"),
    (2, dict(ppd=2048), "PPD = 2048"),
    (2, dict(ppd=96), "PPD = 96"),
]


@pytest.mark.parametrize("order,kw,word", REFUSED, ids=[r[2].replace(" ", "") for r in REFUSED])
def test_refusals(zd, ps, capfd, order, kw, word):
    kw = dict(kw)
    n = kw.pop("ppd", 32)
    field = np.zeros((32, 32, 32), dtype=np.float32)  # (2048: refused by its size before the field is looked at)
    field[1, 2, 3] = 1.0
    if n == 96:
        field = np.zeros((96, 96, 96), dtype=np.float32)
    p = zd.make_params(n, boxsize=BOX, **kw)
    capfd.readouterr()
    with pytest.raises(RuntimeError):
        zd.generate_field(p, ps, field, order=order)
    line = _one_field_line(capfd.readouterr().err, word)
    print(line)
    if n == 2048:
        assert re.search(r"27\d GB", line), line
    with pytest.raises(RuntimeError):
        zd.Plan.from_field(p, ps, field, order=order)
    _one_field_line(capfd.readouterr().err, word)


def test_order_one_is_the_call_without_the_keyword(zd, ps):
    n = 32
    p = zd.make_params(n, boxsize=BOX)
    assert zd.generate_field(p, ps, _noise(n), order=1)["records"].tobytes() == zd.generate_field(p, ps, _noise(n))["records"].tobytes()
    plan = zd.Plan.from_field(p, ps, _noise(n), order=1)
    try:
        assert plan.narray == 2
    finally:
        plan.close()


# ---- 9. command line -----------------------------------------------------------------------------------------------------------
PAR = """BoxSize = 720
CPD = 5
ICFormat = "RVdoubleZel"
InitialConditionsDirectory = "%(out)s"
InitialRedshift = 49
NP = %(np)d
ZD_NumBlock = 2
ZD_Pk_filename = "%(pk)s"
ZD_Pk_norm = 8.0
ZD_Pk_scale = 1.0
ZD_Pk_sigma = 0.0210839935761
ZD_Pk_smooth = 0.0
ZD_Seed = 12346
ZD_qdensity = 0
ZD_Version = 2
"""


def test_command_line(zd, ps, tmp_path):
    n = 32
    a64 = _noise(n).astype(np.float32).astype(np.float64)
    a64.tofile(tmp_path / "a.f64")
    out = tmp_path / "ic"
    out.mkdir()
    par = tmp_path / "f.par"
    head = PAR % dict(out=out, pk=WMAP, np=n ** 3) + 'ZD_Field_filename = "%s"\n' % (tmp_path / "a.f64")

    def run(extra):
        par.write_text(head + extra)
        return subprocess.run([EXE, str(par)], capture_output=True, text=True)

    r = run("ZD_Field_order = 2\n")
    assert r.returncode == 0, r.stderr
    assert "field: density, float64, PPD 32, order 2" in r.stderr.splitlines(), r.stderr
    files = b"".join((out / ("ic_%d" % i)).read_bytes() for i in range(5))
    want = zd.generate_field(zd.make_params(n, boxsize=BOX, cpd=5), ps, a64, order=2)["records"].tobytes()
    assert files == want and files != zd.generate_field(zd.make_params(n, boxsize=BOX, cpd=5), ps, a64)["records"].tobytes()
    r = run("ZD_Field_order = 1\n")
    assert r.returncode == 0 and "field: density, float64, PPD 32" in r.stderr.splitlines(), r.stderr
    r = run("ZD_Field_order = 3\n")
    assert r.returncode == 1, (r.returncode, r.stderr)
    _one_field_line(r.stderr, "order = 3")
    r = run("ZD_Field_order = 2\nZD_q2LPT = 1\n")
    assert r.returncode == 1, (r.returncode, r.stderr)
    _one_field_line(r.stderr, "ZD_q2LPT")


# ---- 10. launch sites (after the tests above) ----------------------------------------------------------------------------------
def test_every_launch_site_was_launched(zd):
    """both instances of the new generator's table have been launched by the tests of this file"""
    txt = open(os.path.join(ROOT, "zeldovich_plt_amd", "csrc", "zd_kernels_lpt2_field.hip")).read()
    assert txt.count("ZD_LAUNCH_CHECK();") == 1
    table = re.search(r"int launch_gen_lpt2_field\(.*?\n}\n", txt, re.S).group(0)
    njs = re.findall(r"launch_gen_lpt2_field_t<(\d+)>", table)
    assert njs == ["2", "7"]
    names = [name for (name, _l), cnt in zd.dispatch_report().items() if cnt > 0]
    for nj in njs:
        assert any("launch_gen_lpt2_field_t" in nm and "NJ = %s" % nj in nm for nm in names), "k_gen_lpt2_field<%s> never launched" % nj
