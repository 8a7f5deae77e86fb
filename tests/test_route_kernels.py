"""Every job zd::route accepts has a kernel at every stage (no GPU).

zd::route (csrc/zd_route.h) decides which jobs the library takes; the launchers' dispatch tables decide what can run.  The hook
zd_test_route_kernels lists, for a job as given, the table every stage consults with its key and the answer of that table's predicate
(csrc/zd_tables.h: the launcher itself, run under a probe up to the point where it would launch) — computed from the job's shape,
whatever route() says.  This sweep asks that no job route() accepts has a stage without a kernel, and that every refusal route() adds
for that reason names the stage.  The set of disagreements is empty: what the sweep finds is fixed in route(), not listed here.

The grid: every power of two 32 ... 16384; every composite PPD of the kernel table (probed, as tests/test_route_agreement.py does);
the even sizes 8 ... 130 and 1000, 2000, 5000, 8190 for the convolutions.  Per size: no stream factor given and every one the family
could take, given (powers of two down to z lines of 8; every divisor of a composite or convolution size that leaves z lines of 3 —
the even ones are the composite kernels', all of them the reference arrays'); ranks 1, 2, 4, 8, 16; and the options below.

Thinned only where two options cannot interact in the route (csrc/zd_route.h, line by line):
- ZD_f_NL != 0 puts the job on the reference's arrays whatever ZD_StoreMode says, and asks only whether it is `reference`
  (fnl_multi_refusal): with f_NL, store modes auto and reference only.
- ZD_qoneslab >= 0 does the same (pack_mode, composite_options): store modes auto and reference only.
- ZD_qdensity = 2 clears ZD_qPLT before the route sees it (canonical): not crossed with qPLT = 1.
- ZD_CornerModes enters through nyquist_dead alone, which k_cutoff = 1 decides by itself: corner_modes = 1 with k_cutoff = 2 only.
- the LPT options are refused by their parameters off the powers of two 32 ... 2048, with ZD_qPLT, ZD_f_NL, a density output,
  ZD_Version = 1 or several ranks (lpt2_refusal): swept on those sizes with those options off, on one rank and on two (the refusal).
- ZD_Version = 1 with the LPT options: refused outright (same function)."""
import ctypes as C
import itertools

FNL = dict(f_NL=2.0e4, n_s=0.96, Omega_M=0.31)
FAM_COMPOSITE, FAM_REF_COMPOSITE = 1, 2
RANKS = (1, 2, 4, 8, 16)
POW2 = [1 << k for k in range(5, 15)]
CONVOLUTION = list(range(8, 131, 2)) + [1000, 2000, 5000, 8190]


def _route(zd, p, R, nranks):
    """the main-pass route of the job as zd_test_route gives it, and its refusal"""
    T = zd.load_testing_library()
    T.zd_test_route.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_char_p, C.c_int64]
    v, why = (C.c_int32 * 12)(), C.create_string_buffer(400)
    T.zd_test_route(C.byref(p), R, nranks, v, why, len(why))
    return dict(zip("family pack narray pstep npass R L Hq Zq dens dens_only twr".split(), v)), why.value.decode()


def _composite_sizes(zd):
    """every PPD <= 8640 the composite kernels know, found by probing (as tests/test_route_agreement.py does): ZA runs on them, or
    ZD_f_NL takes the composite transforms"""
    return [n for n in range(6, 8641, 2)
            if n & (n - 1) and (_route(zd, zd.make_params(n), 0, 1)[0]["family"] == FAM_COMPOSITE
                                or _route(zd, zd.make_params(n, **FNL), 0, 1)[0]["family"] == FAM_REF_COMPOSITE)]


def _factors(n):
    if n & (n - 1) == 0:
        return [0] + [1 << k for k in range(0, 15) if n >> k >= 8]
    return [0] + [r for r in range(1, n // 3 + 1) if n % r == 0]


def _options():
    for sm, fnl, one in itertools.product(("auto", "reference", "packed", "fields"), (0, 1), (-1, 0)):
        if (fnl or one >= 0) and sm in ("packed", "fields"):
            continue
        for (plt, dens), (kc, cm), ver in itertools.product(((0, 0), (0, 1), (0, 2), (1, 0), (1, 1)), ((1.0, 0), (2.0, 0), (2.0, 1)), (2, 1)):
            yield dict(store_mode=sm, qoneslab=one, qPLT=plt, qdensity=dens, k_cutoff=kc, corner_modes=cm, version=ver, **(FNL if fnl else {}))


def _lpt_options():
    for sm, one, (kc, cm) in itertools.product(("auto", "reference", "packed", "fields"), (-1, 0), ((1.0, 0), (2.0, 0), (2.0, 1))):
        for lpt in (dict(q2LPT=1), dict(q2LPT=1, lpt2_dealias=1), dict(q2LPT=1, q3LPT=1)):
            yield dict(store_mode=sm, qoneslab=one, k_cutoff=kc, corner_modes=cm, **lpt)


def sweep(zd, sizes=None, max_ppd=None):
    """(ppd, options, stream factor, ranks, code of zd_test_route_kernels) for every job of the grid"""
    comp = _composite_sizes(zd)
    assert len(comp) >= 55 and 96 in comp and 6912 in comp and 8640 in comp
    grid = sorted(set(POW2 + comp + CONVOLUTION)) if sizes is None else sizes
    for n in grid:
        if max_ppd and n > max_ppd:
            continue
        rs = _factors(n)
        jobs = [(kw, RANKS) for kw in _options()]
        if n in POW2 and n <= 2048:
            jobs += [(kw, (1, 2)) for kw in _lpt_options()]
        for kw, ranks in jobs:
            p = zd.make_params(n, **kw)
            for R in rs:
                p.stream_factor = R
                for G in ranks:
                    yield n, kw, R, G, zd.test_route_kernels(p, R, G, text=False)


def _name(zd, n, kw, R, G):
    r = zd.test_route_kernels(zd.make_params(n, stream_factor=R, **kw), R, G)
    lacking = [s for s in r["stages"] if not s[3]]
    return "PPD %d %s R=%d ranks=%d: %s | %s" % (n, {k: v for k, v in kw.items() if k not in ("n_s", "Omega_M")}, R, G, lacking, r["why"])


def test_every_accepted_job_has_a_kernel_at_every_stage(capfd):
    import zeldovich_plt_amd.api as zd
    asked = accepted = 0
    holes, refused = [], []
    for n, kw, R, G, code in sweep(zd):
        asked += 1
        assert code >= -2, (n, kw, R, G, code)
        if code >= 0:
            accepted += 1
            if code > 0:
                holes.append((n, kw, R, G))
        elif code == -2:
            refused.append((n, kw, R, G))
    capfd.readouterr()
    print("route x kernels: %d jobs asked, %d accepted, %d refused because a stage has no kernel" % (asked, accepted, len(refused)))
    assert asked > 1000000 and accepted > 100000
    first = {}   # one job per size and option set
    for h in holes:
        first.setdefault((h[0], tuple(sorted((k, str(v)) for k, v in h[1].items() if k not in ("k_cutoff", "corner_modes", "version")))), h)
    assert not holes, "%d accepted jobs lack a kernel at a stage, e.g.\n%s" % (len(holes), "\n".join(_name(zd, *h) for h in list(first.values())[:40]))
    # every refusal of this kind names the stage, the launcher and the key; nothing else in the route words a refusal this way
    seen = set()
    for n, kw, R, G in refused:
        key = (n, kw["qPLT"] if "qPLT" in kw else 0, kw.get("store_mode"), bool(kw.get("f_NL")), G > 1)
        if key in seen:
            continue
        seen.add(key)
        r = zd.test_route_kernels(zd.make_params(n, stream_factor=R, **kw), R, G)
        lacking = [s for s in r["stages"] if not s[3]]
        assert not r["accepted"] and lacking, (n, kw, R, G, r)
        stage, launcher, key_, _ = lacking[0]
        assert r["why"] == "PPD = %d: no kernel for the %s stage of this job (%s, %s): it is refused at plan creation" % (n, stage, launcher, key_), r
    # the ones the issue names: the PLT field store below PPD 64 on any rank count, ZD_f_NL at PPD 8192 on one rank
    got = {(n, G) for n, kw, R, G in refused if kw.get("qPLT") and kw["store_mode"] == "fields"}
    assert {(32, G) for G in (1, 2)} <= got and all(n < 64 for n, _ in got), sorted(got)
    assert any(n == 8192 and kw.get("f_NL") and G == 1 for n, kw, R, G in refused)


def test_the_other_roles_and_the_demotion(capfd):
    """The phi pass, the second f_NL pass and the gradient passes asked by themselves: the same property; and the demotion of a field
    store whose rows per rank are no whole row blocks stays a demotion (an accepted job on the packed arrays), not a refusal."""
    import zeldovich_plt_amd.api as zd
    for n in POW2 + [96, 1728, 6912, 100, 1000]:
        for role, kw in (("phi", FNL), ("phik", FNL), ("lpt2_grad", dict(q2LPT=1))):
            for G in (1, 2, 8):
                p = zd.make_params(n, **kw)
                code = zd.test_route_kernels(p, 1 if role != "phik" else 0, G, role=role, text=False)
                assert code <= 0, (n, role, G, zd.test_route_kernels(p, 1 if role != "phik" else 0, G, role=role))
    for kw, G, packed in ((dict(qPLT=1, store_mode="fields"), 4, 2), (dict(qPLT=1, store_mode="fields"), 8, 2), (dict(), 8, 1)):
        p = zd.make_params(64, stream_factor=2, **kw)
        rt, why = _route(zd, p, 2, G)
        want = packed if G == 8 else (4 if kw else 3)  # 4 rows per rank: the packed arrays; 8: one row block, the field store
        assert why == "" and rt["pack"] == want, (kw, G, rt, why)
    capfd.readouterr()
