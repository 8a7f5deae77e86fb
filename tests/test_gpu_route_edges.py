"""GPU: the small edges of the set of jobs zd::route accepts, each against the oracle, and what each really launches against what
zd_test_route_kernels predicted for it (csrc/zd_route.h route_stages).

The case list is computed, not written down: the accepted set of the host sweep (tests/test_route_kernels.py) at PPD <= 256 on 1 ... 8
ranks, ZD_Version = 2, no ZD_qoneslab (both leave the tuples below unchanged: they pick streams and delivered planes, not kernels'
sizes); for every distinct (family, store, arrays, ZA / PLT, density mode, f_NL) that occurs, the smallest PPD, there the largest
stream factor (the shortest z lines), there the largest rank count (the fewest rows and planes per rank) and the one just below it.
Added, each the smallest job of the same sweep: where a field store is asked for (ZA, PLT, with and without a density), the rank
count at which the route demotes it to the packed arrays and the one just below it, which keeps it; ZD_f_NL on one rank and on two
per family (the single-rank phi round — launch_fnl_t, or the half-space planes of the composite transforms — and the phi round of
the smallest group); ZD_Version = 1 per family.  Each case runs
zd.generate (ngpu = ranks, one group) and compares with oracle.run on the same seed as _compare of tests/test_gpu_parity.py does:
indices exact, float64 fields <= 1e-10 of the field maximum, density planes <= 1e-6, density_variance and max_disp <= 1e-10, every
plane seen once.  Around the run the difference of zd_dispatch_report must hold every predicted launcher with its key, and no z / y /
x launcher that was not predicted.

The LPT family: the smallest accepted ZD_q2LPT and ZD_q3LPT jobs at their largest stream factor — z lines of 16 points, which only
their final passes run — compared as tests/test_gpu_lpt2.py / test_gpu_lpt3.py do: the numpy restatements on oracle records with those
files' SIGMA, the higher-order part alone to 1e-10 of its own maximum.  (ZD_2LPT_dealias is not among them: its round has no edge in
the route that tests/test_gpu_lpt2_dealias.py does not run.)

Not held to a launch here: the fused generator + z FFT branch of plan_stages (launch_genz_t and the plane-interleaved y and x stages of
the packed PLT store).  genz_plt_supported starts at PPD 512, above these cases, and check_dispatch matches a launcher by the prefix
of its name and its first size, which does not tell the fused y / x stages from the plain ones.  tests/test_gpu_fused_z.py and
tests/test_zz_dispatch_coverage.py run those kernels; that restatement is checked by the host sweep's predicates alone.

The cases run in child processes, one per family; a child writes one JSON line per finished case and stops at the first case that
does not return; after a child that was killed, died on a signal or reported a HIP error nothing more is started."""
import json
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT, WMAP

FAMILIES = ["pow2", "composite", "ref_composite", "convolution", "lpt"]
FNL = dict(f_NL=2.0e4, n_s=0.96, Omega_M=0.31)
# seconds: ten times the measured wall time of a child, not below 60.  Measured on an MI355X, first clean run: pow2 3.5 s (34 cases),
# composite 3.4 s (9), ref_composite 5.3 s (13), convolution 2.2 s (11), lpt 2.3 s (2)
CHILD_TIMEOUT = {f: 60 for f in FAMILIES}
TOL64, TOL32 = 1e-10, 1e-6
FIELD_PACKS = (3, 4)    # PACK_ZAFIELD, PACK_PLTFIELD (csrc/zd_device.h)
_CASES = {}


def _tuple_of(rt, kw):
    return (rt["family"], rt["pack"], rt["narray"], int(kw.get("qPLT", 0)), int(kw.get("qdensity", 0)), bool(kw.get("f_NL")))


def case_list():
    """(cases, tuples of the whole accepted set): a case = dict(ppd, kw, R, ranks, tuple)"""
    if _CASES:
        return _CASES["cases"], _CASES["tuples"]
    import zeldovich_plt_amd.api as zd
    import test_route_kernels as trk
    best, lpt, fnl, v1, asked = {}, {}, {}, {}, {}
    for n, kw, R, G, code in trk.sweep(zd, max_ppd=256):
        if code == 0 and kw.get("q2LPT") and not kw.get("lpt2_dealias") and kw["store_mode"] == "auto" and kw["qoneslab"] < 0 and kw["k_cutoff"] == 1.0:
            order = 3 if kw.get("q3LPT") else 2
            if order not in lpt or (n, -R) < (lpt[order]["ppd"], -lpt[order]["R"]):
                lpt[order] = dict(ppd=n, kw=dict(q2LPT=1, **({"q3LPT": 1} if order == 3 else {})), R=R, ranks=G, tuple=None, lpt=order)
        if code != 0 or G > 8 or kw.get("qoneslab", -1) >= 0 or kw.get("q2LPT"):
            continue
        p = zd.make_params(n, stream_factor=R, **kw)
        rt, why = trk._route(zd, p, R, G)
        assert why == ""
        t = _tuple_of(rt, kw)
        rank_of = (n, -rt["R"])
        job = dict(ppd=n, kw=kw, R=rt["R"], ranks=G, tuple=list(t))
        if kw.get("version", 2) != 2:
            if t[0] not in v1 or rank_of + (G,) < v1[t[0]]["rank_of"]:   # the smallest ZD_Version = 1 job of each family: PPD, z lines, ranks
                v1[t[0]] = dict(rank_of=rank_of + (G,), job=dict(job, tuple=None, family=t[0]))
            continue
        cur = best.setdefault(t, {})
        if not cur or rank_of < cur["rank_of"]:
            cur.clear()
            cur.update(rank_of=rank_of, jobs={})
        if rank_of == cur["rank_of"]:
            cur["jobs"].setdefault(G, job)
        if kw.get("f_NL") and G <= 2:                         # ZD_f_NL on one rank and on two, per family: the phi round of few ranks
            cur = fnl.setdefault((t[0], G), {})
            if not cur or rank_of < cur["rank_of"]:
                cur.update(rank_of=rank_of, job=dict(job, tuple=None, family=t[0]))
        if kw["store_mode"] == "fields":                      # a field store asked for: the store every rank count gets
            asked.setdefault((t[0], t[3], t[4]), {}).setdefault(rank_of, {}).setdefault(G, (rt["pack"], dict(job, tuple=None, family=t[0])))
    cases = []
    for t, cur in sorted(best.items()):
        gs = sorted(cur["jobs"])
        for G in gs[-2:]:          # the largest rank count and the one just below it
            cases.append(cur["jobs"][G])
    for key in sorted(fnl):
        cases.append(fnl[key]["job"])
    demoted = {}
    for key, sizes in sorted(asked.items()):
        for rank_of in sorted(sizes):                         # the smallest job at which the request is kept on few ranks, demoted on more
            by_g = sizes[rank_of]
            gs = sorted(by_g)
            drop = [(a, b) for a, b in zip(gs, gs[1:]) if by_g[a][0] in FIELD_PACKS and by_g[b][0] not in FIELD_PACKS]
            if drop:
                demoted[key] = [by_g[g][1] for g in drop[0]]  # the rank count just below the demotion, and the demoted one
                cases += demoted[key]
                break
    cases += [v1[fam]["job"] for fam in sorted(v1)] + [lpt[2], lpt[3]]
    seen, out = set(), []
    for c in cases:                # a job two rules chose runs once (the cases of the tuples come first)
        if job_key(c) not in seen:
            out.append(c)
        seen.add(job_key(c))
    _CASES.update(cases=out, tuples=set(best), fnl={k: v["job"] for k, v in fnl.items()}, demoted=demoted, v1={k: v["job"] for k, v in v1.items()})
    return out, set(best)


def job_key(c):
    return json.dumps([c["ppd"], sorted(c["kw"].items()), c["R"], c["ranks"]])


def family_of(case):
    return "lpt" if case.get("lpt") else FAMILIES[case["tuple"][0] if case["tuple"] else case["family"]]


def test_the_case_list_covers_the_accepted_set():
    """every (family, store, arrays, ZA / PLT, density mode, f_NL) of the accepted set has a case — a condition computed from the sweep —
    and no case is larger than PPD 256"""
    cases, tuples = case_list()
    assert tuples and {tuple(c["tuple"]) for c in cases if c["tuple"]} == tuples
    assert {t[0] for t in tuples} == {0, 1, 2, 3}                 # all four families occur
    assert all(c["ppd"] <= 256 for c in cases) and len(cases) <= 80, len(cases)
    assert sorted(c["lpt"] for c in cases if c.get("lpt")) == [2, 3] and all(c["ppd"] // c["R"] == 16 for c in cases if c.get("lpt"))
    # the added jobs, each the smallest of the accepted set: ZD_f_NL on one rank and on two for every family that takes it there (the
    # powers of two and the composite transforms of the reference's arrays on both), ZD_Version = 1 per family, and for a field store
    # asked for, ZA and PLT, the rank count at which it is demoted and the one just below it
    have = {job_key(c) for c in cases}
    fnl, demoted, v1 = _CASES["fnl"], _CASES["demoted"], _CASES["v1"]
    assert {(0, 1), (0, 2), (2, 1), (2, 2)} <= set(fnl) and all(job_key(j) in have and j["kw"]["f_NL"] and j["ranks"] == G for (_, G), j in fnl.items())
    assert set(v1) == {0, 1, 2, 3} and all(job_key(j) in have and j["kw"]["version"] == 1 for j in v1.values())
    assert {(0, 0, 0), (0, 1, 0)} <= set(demoted), sorted(demoted)     # (family, ZA / PLT, density mode)
    for below, at in demoted.values():
        assert job_key(below) in have and job_key(at) in have and below["kw"]["store_mode"] == at["kw"]["store_mode"] == "fields"
    print("%d edge cases: %s" % (len(cases), {f: sum(family_of(c) == f for c in cases) for f in FAMILIES}))


def _size_of(targs):
    d = dict(re.findall(r"(\w+) = (\w+)", targs))
    for k in ("L", "N", "M"):
        if k in d:
            return int(d[k])
    return int(d["P"]) * int(d["Q"]) if "P" in d and "Q" in d else None


def check_dispatch(stages, launched):
    """stages: [(stage, launcher, key, present)] predicted; launched: names of the launch sites that counted launches in the run"""
    tracked = re.compile(r"launch_(zfft|yfft|xfft|xdens|fnl|genz|refq_(cols|lines|ycols|yphi|xphi)|any_(cols|lines)|lpt)")
    seen = []
    for name in launched:
        m = re.search(r"(launch_\w+)\(.*\[(.*)\]\s*$", name)
        if m and tracked.match(m.group(1)):
            seen.append((m.group(1), _size_of(m.group(2)), m.group(2)))
    want = [(launcher, int(re.search(r"\d+", key).group(0)), key) for _s, launcher, key, _p in stages]
    missing = [w for w in want if not any(s[0].startswith(w[0]) and s[1] == w[1] for s in seen)]
    extra = [s for s in seen if not any(s[0].startswith(w[0]) and s[1] == w[1] for w in want)]
    return missing, extra


def _rel(a, b):
    import numpy as np
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def run_lpt_case(zd, oracle, case):
    """the higher-order part alone against the numpy restatement on oracle records, as tests/test_gpu_lpt2.py / test_gpu_lpt3.py do"""
    import numpy as np
    import lpt2_ref
    import lpt3_ref
    n, R, order = case["ppd"], case["R"], case["lpt"]
    sigma = 0.42 if order == 2 else 0.84       # SIGMA of tests/test_gpu_lpt2.py, tests/test_gpu_lpt3.py
    rec = oracle.run(oracle.make_params(n), oracle.pk_from_file(WMAP, 720.0, Pk_sigma=sigma))["records"]
    q = np.ascontiguousarray(rec["d"], dtype=np.float64)
    alive = lpt2_ref.alive_mask(n, 720.0, 1.0)
    ps = zd.PowerSpectrum.from_file(WMAP, 720.0, Pk_sigma=sigma)
    # the order below: the ZA run (at its own stream factor: its z lines start at 32) or the second-order run at the same one
    lower = zd.generate(zd.make_params(n) if order == 2 else zd.make_params(n, stream_factor=R, q2LPT=1), ps)["records"]
    p = zd.make_params(n, stream_factor=R, **case["kw"])
    pred = zd.test_route_kernels(p, R, 1)
    assert pred["code"] == 0, pred
    before = zd.dispatch_report()
    got = zd.generate(p, ps)
    after = zd.dispatch_report()
    assert sorted(got["planes_seen"]) == list(range(n)) and got["stream_factor"] == R, "planes seen"
    g = got["records"]
    if order == 2:
        ref = (3.0 / 7.0) * lpt2_ref.second_order(q, 720.0, alive, lpt2_ratio=-1.0)    # gamma = 3/7 at f_cluster = 1
        part_d, part_v, f = g["d"] - lower["d"], g["v"] - 1.0 * lower["d"], 2.0
    else:
        ref = lpt3_ref.combine(lpt3_ref.third_order(q, 720.0, alive))
        part_d, part_v, f = g["d"] - lower["d"], g["v"] - lower["v"], lpt3_ref.DEFAULTS["f3"]
    scale = np.abs(ref).max()
    errs = {"first order": _rel(lower["d"], rec["d"]) if order == 2 else 0.0, "higher-order d": float(np.abs(part_d - ref).max() / scale),
            "higher-order v": float(np.abs(part_v - f * ref).max() / scale)}
    bad = ["%s %.3g" % (k, v) for k, v in errs.items() if not v <= TOL64]
    if not np.array_equal(g["ijk"], lower["ijk"]):
        bad.append("ijk")
    missing, extra = check_dispatch(pred["stages"], [k[0] for k in after if after[k] != before.get(k, 0)])
    if missing:
        bad.append("predicted, not launched: %r" % (missing,))
    if extra:
        bad.append("launched, not predicted: %r" % (extra,))
    return errs, bad


def run_case(zd, oracle, ps, case):
    import ctypes as C
    import numpy as np
    if case.get("lpt"):
        return run_lpt_case(zd, oracle, case)
    n, kw, R, G = case["ppd"], dict(case["kw"]), case["R"], case["ranks"]
    fmt = "RVdoubleZel"
    eig = oracle.synthetic_eigenmodes(32) if kw.get("qPLT") else None
    p = zd.make_params(n, icformat=fmt, stream_factor=R, ngpu=G if G > 1 else 0, pass_groups=1 if G > 1 else 0, **kw)
    pred = zd.test_route_kernels(p, R, G)
    assert pred["code"] == 0, pred
    before = zd.dispatch_report()
    got = zd.generate(p, ps, eig=eig)
    after = zd.dispatch_report()
    launched = [k[0] for k in after if after[k] != before.get(k, 0)]
    okw = {k: v for k, v in kw.items() if k not in ("store_mode",)}
    if "corner_modes" in okw:
        okw["CornerModes"] = okw.pop("corner_modes")
    opk = oracle.pk_from_file(WMAP, 720.0)
    if kw.get("f_NL"):
        oracle.lib().zdo_pk_set_primordial(C.byref(opk), kw["n_s"])
    ref = oracle.run(oracle.make_params(n, numblock=2, icformat=fmt, **okw), opk, eig=eig, eig_ppd=0 if eig is None else eig.shape[0],
                     want_density=bool(kw.get("qdensity", 0)))
    errs, bad = {}, []
    assert sorted(got["planes_seen"]) == list(range(n)), "planes seen"
    if ref["records"] is not None:
        g, r = got["records"], ref["records"]
        if not np.array_equal(g["ijk"], r["ijk"]):
            bad.append("ijk")
        for f in ("d", "v"):
            errs[f] = max(_rel(g[f][..., c], r[f][..., c]) for c in range(3))
        errs["max_disp"] = _rel(got["max_disp"], ref["max_disp"])
        for j in range(3):
            col = g["d"][..., 2 - j].ravel()
            first = int(np.argmax(np.abs(col))) if np.any(col) else -1
            if got["max_disp_index"][j] != first:
                bad.append("max_disp_index[%d]" % j)
    if ref["density"] is not None:
        errs["density"] = _rel(got["density"], ref["density"])
    errs["density_variance"] = abs(got["density_variance"] - ref["density_variance"]) / ref["density_variance"]
    for k, v in errs.items():
        if not v <= (TOL32 if k == "density" else TOL64):
            bad.append("%s %.3g" % (k, v))
    missing, extra = check_dispatch(pred["stages"], launched)
    if missing:
        bad.append("predicted, not launched: %r" % (missing,))
    if extra:
        bad.append("launched, not predicted: %r" % (extra,))
    return errs, bad


def child_main(family, cases_path, out_path):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import time
    import zeldovich_plt_amd.api as zd
    from oracle import zdo
    zdo.build()
    cases = [c for c in json.load(open(cases_path)) if family_of(c) == family]
    ps = zd.PowerSpectrum.from_file(WMAP, 720.0)
    with open(out_path, "w") as f:
        for i, case in enumerate(cases):
            t0 = time.time()
            rec = dict(family=family, index=i, case=case)
            try:
                rec["errs"], rec["bad"] = run_case(zd, zdo, ps, case)
            except AssertionError as e:
                rec["errs"], rec["bad"] = {}, ["assertion: %s" % (e,)]
            except RuntimeError as e:      # the library refused or failed: nothing more on the card from this child
                rec["errs"], rec["bad"], rec["fatal"] = {}, ["did not return a result: %s" % (e,)], True
            rec["seconds"] = time.time() - t0
            f.write(json.dumps(rec) + "\n")
            f.flush()
            if rec.get("fatal"):
                return 3
    return 0


def _run_family(family, tmp_path):
    out = tmp_path / ("%s.jsonl" % family)
    import time
    t0 = time.time()
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--family", family, "--cases", str(tmp_path / "cases.json"), "--out", str(out)],
                           capture_output=True, text=True,
                           timeout=CHILD_TIMEOUT[family], cwd=ROOT)
        rc, err = r.returncode, r.stderr
    except subprocess.TimeoutExpired as e:
        rc, err = 124, (e.stderr or b"").decode(errors="replace") if isinstance(e.stderr, bytes) else (e.stderr or "")
    recs = [json.loads(ln) for ln in out.read_text().splitlines()] if out.exists() else []
    return rc, err, recs, time.time() - t0


@pytest.mark.gpu
def test_route_edges_against_the_oracle(tmp_path):
    cases, _ = case_list()
    (tmp_path / "cases.json").write_text(json.dumps(cases))
    failures, stop = [], None
    for family in FAMILIES:
        want = sum(family_of(c) == family for c in cases)
        rc, err, recs, wall = _run_family(family, tmp_path)
        worst = {}
        for rec in recs:
            for k, v in rec["errs"].items():
                worst[k] = max(worst.get(k, 0.0), v)
            if rec["bad"]:
                failures.append((family, rec["case"], rec["bad"]))
        print("route edges, %s: %d of %d cases, child wall time %.1f s, worst errors %s" % (family, len(recs), want, wall,
                                                                                           {k: "%.2g" % v for k, v in worst.items()}))
        hip_error = "illegal memory access" in err or "hipError" in err or "HSA_STATUS_ERROR" in err
        if rc < 0 or rc in (124, 134, 137, 139) or hip_error:
            stop = "child %s ended with status %d%s after %d of %d cases; the remaining families were not started\n%s" % (
                family, rc, " and a HIP error" if hip_error else "", len(recs), want, err[-1500:])
            break
        if rc != 0 or len(recs) != want:
            failures.append((family, "child status %d, %d of %d cases" % (rc, len(recs), want), err[-1500:]))
    assert stop is None, stop
    assert not failures, "\n".join(repr(f) for f in failures)


if __name__ == "__main__":
    a = sys.argv
    sys.exit(child_main(a[a.index("--family") + 1], a[a.index("--cases") + 1], a[a.index("--out") + 1]))
