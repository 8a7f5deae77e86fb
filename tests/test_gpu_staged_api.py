"""The staged API (include/zeldovich_hip.h: zd_plan_stage_z / _y / _x, zd_plan_stats) under every legal call order.

The plan carries state from one call to the next — the generator's slab ring and its run-ahead (`ahead_pass`, `ahead_g0`,
`ahead_n`, `next_g`), the once-per-run variance flag `var_pending`, the density planes of PLT + ZD_qdensity = 1 on composite grids
(`d_dens_pass`) — and the header asks for no particular order.  Every plan family the dispatcher builds runs here under

  O1  canonical: one store, passes ascending, one stage_x over the whole pass (the reference for the others);
  O2  two stores in flight: stage_z(p + 1, B) is issued before stage_y / stage_x of pass p on A, the stores alternating;
  O3  the passes in reverse;
  O4  a seeded permutation of the passes, one of them with its Z stage run twice (the second time into the other store);
  O5  stage_x in pieces (multiples of plane_step, odd numbers of steps among them), the last piece first, each into its own buffer;
  O6  every call on one non-default caller stream, one synchronisation at the end;
  O7  (families with the generator's worker streams and a packed / field store) plan.stats() after every pass;

and must give byte-identical records and density planes, identical max_disp / max_disp_index and the same density_variance (1e-13:
the atomic sum's order is free) as O1.  O1 itself is anchored to the CPU oracle with the tolerances of test_gpu_parity.py::_compare
and must equal zd_generate byte for byte.

Run-ahead: the product library's slab ring has K = 2 slots for every plan (a deeper ring is a -DZD_TUNING experiment), so the
generator never runs ahead into the next pass there; test_run_ahead_with_a_deeper_ring repeats O7 through the tuning build with
four slots, where it does.
"""
import collections
import concurrent.futures
import contextlib
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, WMAP, source_sha

pytestmark = pytest.mark.gpu

TOL = 1e-10          # f64 records against the oracle (test_gpu_parity.py)
VAR_TOL = 1e-13      # density_variance between call orders
PLT = dict(qPLT=1, qPLTrescale=1, PLT_target_z=5.0, f_cluster=0.97)
FNL = dict(f_NL=2.0e4, n_s=0.96, Omega_M=0.31)

Family = collections.namedtuple("Family", "n fmt kw plt eig_ppd expect o7 oracle")
# expect = (store_mode, plane_step, passes); o7: the plan has the generator's worker streams and a packed / field store (its
# density_variance comes from sum |D|^2 in the Z stage, so every stats() read must report all of it); oracle: the oracle run
# that anchors O1 (the three composite ZA families share one: records, density planes and variance are the same numbers)
FAMILIES = {
    "p2_reference":      Family(128, "RVdoubleZel", dict(store_mode="reference", stream_factor=4), False, 0, ("reference", 1, 4), False, "own"),
    "p2_packed_pairs":   Family(256, "RVdoubleZel", dict(store_mode="packed", stream_factor=8), False, 0, ("packed", 2, 4), True, "own"),
    "p2_za_fields":      Family(256, "RVdoubleZel", dict(stream_factor=8), False, 0, ("fields", 2, 4), True, "own"),
    "p2_plt_two_kernel": Family(128, "RVdoubleZel", dict(store_mode="packed", stream_factor=4), True, 32, ("packed", 1, 4), True, "own"),
    # the fused generator + z FFT takes z lines of 512 or 1024 with PPD = L or 2L: two passes at most (PPD = 1024, R = 2); too large for
    # the oracle here, it is anchored through zd_generate, which the suite ties to the oracle at 512 and to the direct sum at 2048
    "p2_plt_fused":      Family(1024, "ZelSimple", dict(stream_factor=2), True, 128, ("packed", 1, 2), False, None),
    # composite grids: z lines of 24 = 8 * 3 (R = 8, two residues per pass: four passes)
    "np2_za_fields":     Family(192, "RVdoubleZel", dict(stream_factor=8), False, 0, ("fields", 2, 4), True, "np2_za"),
    "np2_za_density":    Family(192, "RVdoubleZel", dict(qdensity=1, stream_factor=8), False, 0, ("fields", 2, 4), True, "np2_za"),
    "np2_density_only":  Family(192, "RVdoubleZel", dict(qdensity=2, stream_factor=8), False, 0, ("fields", 2, 4), True, "np2_za"),
    # PLT + density: the density-only sub-plan (R = 8, z lines of 24) at the head of every Z stage of the PLT plan (R = 4, lines of 48)
    "np2_plt_dens_sub":  Family(192, "RVdoubleZel", dict(qdensity=1, stream_factor=4), True, 32, ("fields", 1, 4), True, "own"),
    "any_conv":          Family(70, "RVdoubleZel", dict(qdensity=1, stream_factor=5), False, 0, ("reference", 1, 5), False, "own"),
    "v1":                Family(128, "RVdoubleZel", dict(version=1, numblock=4, stream_factor=4, store_mode="reference"), False, 0,
                                ("reference", 1, 4), False, "own"),
    "fnl":               Family(128, "RVdoubleZel", dict(stream_factor=4, **FNL), False, 0, ("reference", 1, 4), False, "own"),
}
ORDERS = ["O1", "O2", "O3", "O4", "O5", "O6", "O7", "oracle"]
CASES = [(f, o) for f in FAMILIES for o in ORDERS if o != "O7" or FAMILIES[f].o7]


@pytest.fixture(scope="module")
def zd():
    import zeldovich_plt_amd.api as api
    api.load_library()
    return api


def _oracle_params(oracle, fam):
    kw = {k: v for k, v in fam.kw.items() if k not in ("stream_factor", "store_mode")}
    if fam.plt:
        kw.update(PLT)
    numblock = kw.pop("numblock", 2)
    return oracle.make_params(fam.n, numblock=numblock, icformat=fam.fmt, **kw)


def _oracle_run(oracle, name):
    """the oracle's run for the family `name` (runs on a worker thread: ctypes releases the GIL, so it overlaps the GPU cases)"""
    fam = FAMILIES[name]
    if fam.oracle == "np2_za":  # the superset of the three: records and density planes
        fam = FAMILIES["np2_za_density"]
    opk = oracle.pk_from_file(WMAP, 720.0)
    if fam.kw.get("f_NL"):
        oracle.lib().zdo_pk_set_primordial(C.byref(opk), fam.kw["n_s"])
    eig = oracle.synthetic_eigenmodes(fam.eig_ppd) if fam.plt else None
    return oracle.run(_oracle_params(oracle, fam), opk, eig=eig, eig_ppd=0 if eig is None else eig.shape[0],
                      want_density=bool(fam.kw.get("qdensity", 0)))


_POOL = concurrent.futures.ThreadPoolExecutor(max_workers=2)
_ORACLE = {}
_EIG = {}
_CUR = {}  # the family whose plan and O1 run are held (one at a time: the fused family's volume is 13 GB)


def _eig(oracle, ppd):
    if ppd not in _EIG:
        _EIG[ppd] = oracle.synthetic_eigenmodes(ppd)
    return _EIG[ppd]


def _family(zd, oracle, name):
    """(plan, params, power spectrum, eigenmodes, O1 run) of the family, made on first use; starts the family's oracle run"""
    import torch
    if _CUR.get("name") != name:
        if _CUR.get("plan") is not None:
            _CUR["plan"].close()
        _CUR.clear()
        torch.cuda.empty_cache()
        fam = FAMILIES[name]
        key = _oracle_key(name)
        if key and key not in _ORACLE:
            _ORACLE[key] = _POOL.submit(_oracle_run, oracle, name)
        ps = zd.PowerSpectrum.from_file(WMAP, 720.0)
        eig = _eig(oracle, fam.eig_ppd) if fam.plt else None
        kw = dict(fam.kw, **(PLT if fam.plt else {}))
        p = zd.make_params(fam.n, icformat=fam.fmt, **kw)
        plan = zd.Plan(p, ps, eig=eig)
        assert (plan.store_mode, plan.plane_step, plan.passes) == fam.expect, (name, plan.store_mode, plan.plane_step, plan.passes)
        assert plan.local_planes * plan.passes == fam.n
        _CUR.update(name=name, plan=plan, params=p, ps=ps, eig=eig)
        fused0 = _fused_launches(zd)
        _CUR["o1"] = _run(zd, plan, fam, "O1")
        fused = _fused_launches(zd) - fused0
        if name == "p2_plt_fused":
            assert fused > 0, "the fused generator + z FFT did not run"
        else:
            assert fused == 0, "the fused Z stage ran for a family that must not take it"
    return _CUR


def _oracle_key(name):
    fam = FAMILIES[name]
    return name if fam.oracle == "own" else fam.oracle


def _dens_sub(fam):
    """PLT + ZD_qdensity = 1 on a composite grid: the plan with the density-only sub-plan"""
    return fam.plt and fam.kw.get("qdensity") == 1 and (fam.n & (fam.n - 1)) != 0


def _fused_launches(zd):
    return sum(cnt for (nm, _l), cnt in zd.dispatch_report().items() if "launch_genz_t" in nm)


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    if _CUR.get("plan") is not None:
        _CUR["plan"].close()
    _CUR.clear()
    import torch
    torch.cuda.empty_cache()


class _Run:
    """one run of a plan through the staged calls: whole-volume records / density planes on the device, every plane once"""

    def __init__(self, plan, fam, stream):
        import torch
        self.torch, self.plan, self.fam, self.n = torch, plan, fam, fam.n
        self.stream = stream
        n = fam.n
        self.has_rec = fam.kw.get("qdensity", 0) != 2
        self.has_dens = fam.kw.get("qdensity", 0) != 0
        import zeldovich_plt_amd.api as api
        self.rs = api.RECORD_DTYPES[fam.fmt].itemsize
        if self.has_rec:
            assert plan.record_size == self.rs
        self.rec = torch.full((n, n * n * self.rs), 255, dtype=torch.uint8, device="cuda") if self.has_rec else None
        self.dens = torch.full((n, n * n), float("nan"), dtype=torch.float32, device="cuda") if self.has_dens else None
        self.seen = []
        self.keep = []  # the buffers of O5's pieces stay alive (distinct buffers) until the run is synchronised

    def store(self):
        s = self.torch.empty(self.plan.exchange_bytes, dtype=self.torch.uint8, device="cuda")
        s.fill_(255)  # NaN bytes: an element nobody wrote shows up in the records
        return s

    def z(self, p, store):
        self.plan.stage_z(p, store.data_ptr(), self.stream)

    def y(self, store):
        self.plan.stage_y(store.data_ptr(), self.stream)

    def x(self, p, store, p0, cnt, density=True):
        torch, n = self.torch, self.n
        rec = torch.empty(cnt * n * n * self.rs, dtype=torch.uint8, device="cuda") if self.has_rec else None
        dens = torch.empty(cnt * n * n, dtype=torch.float32, device="cuda") if (self.has_dens and density) else None
        self.plan.stage_x(p, store.data_ptr(), p0, cnt, None if rec is None else rec.data_ptr(), None if dens is None else dens.data_ptr(),
                          self.stream)
        zs = [self.plan.plane_z(p, p0 + i) for i in range(cnt)]
        idx = torch.tensor(zs, dtype=torch.int64, device="cuda")
        if rec is not None:
            self.rec.index_copy_(0, idx, rec.view(cnt, -1))
        if dens is not None:
            self.dens.index_copy_(0, idx, dens.view(cnt, -1))
        self.keep += [rec, dens]
        self.seen += zs
        return zs

    def pass_(self, p, store, density=True):
        self.y(store)
        return self.x(p, store, 0, self.plan.local_planes, density)


def _run(zd, plan, fam, order, reads=None):
    """run `order`; returns dict(rec, dens, seen, stats, dens_planes = the planes whose density was delivered)"""
    import torch
    P, LP, ps = plan.passes, plan.local_planes, plan.plane_step
    s = torch.cuda.Stream() if order == "O6" else None
    ctx = torch.cuda.stream(s) if s is not None else contextlib.nullcontext()
    dens_planes = None  # None: all
    with ctx:
        r = _Run(plan, fam, s.cuda_stream if s is not None else 0)
        A = r.store()
        if order in ("O1", "O6", "O7"):
            for p in range(P):
                r.z(p, A)
                r.pass_(p, A)
                if order == "O7":
                    reads.append(plan.stats())
        elif order == "O2":
            stores = [A, r.store()]
            dens_sub = _dens_sub(fam)
            r.z(0, stores[0])
            dens_planes = []
            for p in range(P):
                cur = stores[p % 2]
                if p + 1 < P:
                    r.z(p + 1, stores[(p + 1) % 2])
                if dens_sub and p + 1 < P:
                    # PLT + density on a composite grid: the plan holds the density planes of the latest Z stage only, so
                    # pass p's density is refused now (the pass's own rows 0.. of the volumes would take it: in bounds)
                    r.y(cur)
                    with pytest.raises(RuntimeError):
                        r.plan.stage_x(p, cur.data_ptr(), 0, LP, r.rec[0].data_ptr(), r.dens[0].data_ptr(), r.stream)
                    r.x(p, cur, 0, LP, density=False)
                else:
                    dens_planes += r.pass_(p, cur)
        elif order == "O3":
            for p in reversed(range(P)):
                r.z(p, A)
                r.pass_(p, A)
        elif order == "O4":
            stores = [A, r.store()]
            perm = [int(v) for v in np.random.default_rng(1000 + fam.n + P).permutation(P)]
            twice = perm[len(perm) // 2]
            for i, p in enumerate(perm):
                cur = stores[i % 2]
                r.z(p, cur)
                if p == twice:  # the same Z stage again into the other store: what was generated ahead is discarded
                    cur = stores[1 - i % 2]
                    r.z(p, cur)
                r.pass_(p, cur)
        elif order == "O5":
            units, sizes, pieces, u0 = LP // ps, [3, 1, 2], [], 0
            while u0 < units:
                k = min(sizes[len(pieces) % 3], units - u0)
                pieces.append((u0 * ps, k * ps))
                u0 += k
            assert any((k // ps) % 2 for _p0, k in pieces)
            for p in range(P):
                r.z(p, A)
                r.y(A)
                for p0, k in reversed(pieces):
                    r.x(p, A, p0, k)
        else:
            raise AssertionError(order)
    torch.cuda.synchronize()
    st = plan.stats()
    r.keep.clear()
    assert sorted(r.seen) == list(range(fam.n)), order
    return dict(rec=r.rec, dens=r.dens, stats=st, dens_planes=dens_planes)


def _same_as_o1(got, o1, what):
    import torch
    if o1["rec"] is not None:
        assert torch.equal(got["rec"], o1["rec"]), what + ": records differ from O1"
    if o1["dens"] is not None:
        zs = got["dens_planes"]
        if zs is None:
            assert torch.equal(got["dens"], o1["dens"]), what + ": density planes differ from O1"
        else:
            assert zs, what
            idx = torch.tensor(zs, dtype=torch.int64, device="cuda")
            assert torch.equal(got["dens"].index_select(0, idx), o1["dens"].index_select(0, idx)), what + ": density planes differ from O1"
    a, b = got["stats"], o1["stats"]
    assert np.array_equal(a["max_disp"], b["max_disp"]), (what, a["max_disp"], b["max_disp"])
    assert np.array_equal(a["max_disp_index"], b["max_disp_index"]), (what, a["max_disp_index"], b["max_disp_index"])
    assert abs(a["density_variance"] - b["density_variance"]) <= VAR_TOL * abs(b["density_variance"]), \
        (what, a["density_variance"], b["density_variance"])


def _rel(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.mark.parametrize("family,order", CASES, ids=["%s-%s" % c for c in CASES])
def test_call_order(zd, oracle, family, order):
    fam = FAMILIES[family]
    cur = _family(zd, oracle, family)
    plan, o1 = cur["plan"], cur["o1"]
    if order == "O1":  # O1 against itself: a second canonical run on the same plan (nothing left over from the first)
        _same_as_o1(_run(zd, plan, fam, "O1"), o1, "O1 again")
    elif order == "O7":
        _stats_between_passes(zd, plan, fam, o1)
    elif order == "oracle":
        _anchor(zd, oracle, family, cur)
    else:
        _same_as_o1(_run(zd, plan, fam, order), o1, order)


def _stats_between_passes(zd, plan, fam, o1):
    """O7: stats() after every pass of an ascending run.  The packed / field stores take density_variance from sum |D|^2 in the
    first Z stage after a read ("once per run: every pass sees every mode"), so EVERY read reports all of it; max_disp is per read
    and the best over the reads (largest |v|, the smallest lattice index on a tie — output.cpp:190-193) is O1's.
    (The product's slab ring has two slots: nothing was generated ahead when the reads happened.  With the tuning build's
    ZD_Y_SLABS = 4 — test_run_ahead_with_a_deeper_ring — the first slabs of the next pass are generated ahead at every read.)"""
    reads = []
    got = _run(zd, plan, fam, "O7", reads=reads)
    full = o1["stats"]["density_variance"]
    assert len(reads) == plan.passes
    for i, st in enumerate(reads):
        assert abs(st["density_variance"] - full) <= VAR_TOL * abs(full), (i, st["density_variance"], full)
    assert got["stats"]["density_variance"] == 0.0  # (nothing was generated after the last read)
    for j in range(3):
        best_v, best_i = 0.0, -1
        for st in reads:
            v, i = st["max_disp"][j], int(st["max_disp_index"][j])
            if i < 0:
                continue
            if abs(v) > abs(best_v) or (abs(v) == abs(best_v) and (best_i < 0 or i < best_i)):
                best_v, best_i = v, i
        assert best_v == o1["stats"]["max_disp"][j] and best_i == o1["stats"]["max_disp_index"][j], (j, best_v, best_i)
    got["stats"] = o1["stats"]  # (the statistics were checked read by read)
    _same_as_o1(got, o1, "O7")


def _anchor(zd, oracle, family, cur):
    """O1 against the CPU oracle (tolerances of test_gpu_parity.py::_compare) and, byte for byte, against zd_generate"""
    import torch
    fam, o1, n = FAMILIES[family], cur["o1"], FAMILIES[family].n
    dt = zd.RECORD_DTYPES[fam.fmt]
    st = o1["stats"]
    if fam.oracle is None:
        assert fam.n > 512  # (only the fused family is beyond the oracle here)
    else:
        ref = _ORACLE[_oracle_key(family)].result()
        if o1["rec"] is not None:
            g = o1["rec"].cpu().numpy().view(dt).reshape(n, n, n)
            r = ref["records"]
            assert np.array_equal(g["ijk"], r["ijk"])
            for f in ("d", "v"):
                if f in dt.names:
                    tol = TOL if g[f].dtype == np.float64 else 1e-6
                    for c in range(3):
                        assert _rel(g[f][..., c], r[f][..., c]) < tol, (f, c, _rel(g[f][..., c], r[f][..., c]))
            for j in range(3):  # max_disp (x, y, z) against the records (qz, qy, qx): signed value and first index of the largest |q|
                col = g["d"][..., 2 - j].ravel()
                first = int(np.argmax(np.abs(col)))
                assert st["max_disp_index"][j] == first and st["max_disp"][j] == col[first], j
            assert _rel(st["max_disp"], ref["max_disp"]) < TOL
        if o1["dens"] is not None:
            assert _rel(o1["dens"].cpu().numpy().reshape(n, n, n), ref["density"]) < 1e-6
        assert abs(st["density_variance"] - ref["density_variance"]) <= TOL * ref["density_variance"]
    # zd_generate: the same kernels, driven by the library itself
    if n <= 256:
        gen = zd.generate(cur["params"], cur["ps"], eig=cur["eig"])
        if o1["rec"] is not None:
            assert gen["records"].tobytes() == o1["rec"].cpu().numpy().tobytes()
        if o1["dens"] is not None:
            assert gen["density"].tobytes() == o1["dens"].cpu().numpy().tobytes()
    else:
        bad = []

        def take(z, rec):
            plane = torch.from_numpy(np.ascontiguousarray(rec).reshape(-1).view(np.uint8)).to("cuda")
            if not torch.equal(plane, o1["rec"][z]):
                bad.append(z)

        gen = zd.generate_planes(cur["params"], cur["ps"], take, eig=cur["eig"])
        assert gen["planes"] == n and not bad, bad[:8]
    assert np.array_equal(gen["max_disp"], st["max_disp"]) and np.array_equal(gen["max_disp_index"], st["max_disp_index"])
    assert abs(gen["density_variance"] - st["density_variance"]) <= VAR_TOL * abs(st["density_variance"])


def test_run_ahead_with_a_deeper_ring():
    """O7 again through the -DZD_TUNING library with a ring of four slabs (ZD_Y_SLABS = 4): every Z stage then starts generating
    the next pass's first slabs ahead, and a stats() read between two passes must not lose their share of sum |D|^2 (the next Z
    stage accumulates the variance; it may not reuse slabs that were generated without it).  Child process, as the tuning knobs
    live only in that build."""
    if os.environ.get("ZD_STAGED_CHILD"):
        pytest.skip("(the child process itself)")
    lib = os.path.join(ROOT, "zeldovich_plt_amd", "csrc", "build", "libzeldovich_hip_tuning.so")
    assert os.path.exists(lib), "tuning variant not built (make -C zeldovich_plt_amd/csrc tuning; build() does it)"
    assert open(lib + ".srcsha").read().split()[0] == source_sha(), "libzeldovich_hip_tuning.so is older than the kernel sources"
    env = dict(os.environ, ZD_LIB_PATH=lib, ZD_Y_SLABS="4", ZD_STAGED_CHILD="1")
    sel = "O7 and (za_fields or plt_two_kernel or plt_dens_sub)"  # p2_ and np2_za_fields, p2_plt_two_kernel, np2_plt_dens_sub
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", os.path.abspath(__file__), "-k", sel],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    print(r.stdout[-1500:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "4 passed" in r.stdout, r.stdout[-1500:]
