"""Times of the adjoint of a field run (api.field_vjp, csrc/zd_kernels_field_adj.hip) on one MI355X -> profiles/field_vjp_times.jsonl.

    python scripts/field_vjp_times.py [--sizes 512,1024,2048] [--out profiles/field_vjp_times.jsonl]

Kernel time per stage comes from a `rocprofv3 --kernel-trace` run of its own (a fresh child process per variant, ZA and PLT: this file
with --worker), the wall times and the 2048 closed-form error from a run without the profiler.  Next to the kernel times go the bytes
per lattice point by count (the README's accounting of the intake: what each stage must read and write, from the shapes) and the share
of the 8 TB/s peak, the ratio to the intake's kernel time (profiles/field_intake_times.jsonl: one forward chain) and to
zd_stats.seconds_total of generate_field at the same size.  Cotangents and result live on the device: float64 g_q and g_v where they
fit, float32 g_q alone at 2048 (12 N^3 bytes beside H and the float64 result, whose storage serves as T: 189 GB; with g_v as
well the job was refused for memory on the 288 GB card beside the arrays torch holds)."""
import argparse
import csv
import glob
import json
import os
import subprocess
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
BOX, FC = 720.0, 0.9
PLT = dict(qPLT=1, qPLTrescale=1, PLT_target_z=5.0)
REPS = 3


def wave(n):
    """(m, phi): at 2048 the float32-exact wave (values 0 and +-1 only), a generic one elsewhere"""
    return ((n // 4, n // 4, -(n // 4)), 0.0) if n >= 2048 else ((-7, 11, 5), 0.3)


def bytes_per_point(plt, two, esz):
    """by count, per lattice point: x reads whole rows of the interleaved cotangent(s) (3 components, `two` arrays) and writes a
    complex row; y reads it and writes half; z reads the half-space line and writes (first pass) or reads and writes H; the inverse
    is the intake backwards"""
    npass = 3 * ((2 if two else 1) if plt else 1)
    arrays = 1 if plt else (2 if two else 1)
    fwd = npass * (3 * esz * arrays + 16 + 16 + 8 + 8) + 8 + (npass - 1) * 16
    inv = (8 + 8) + (8 + 16) + (16 + 8)
    return fwd + inv, npass


def cases(sizes):
    for n in sizes:
        yield n, (n >= 2048)


def worker(args):
    import torch
    import field_adj_ref
    import zeldovich_plt_amd.api as zd
    ps = zd.PowerSpectrum.from_file(os.path.join(ROOT, "tests", "golden", "wmap1new.pow"), BOX)
    eig = zd.make_eigenmodes(64) if args.plt else None
    for n, lean in cases(args.sizes):
        p = zd.make_params(n, boxsize=BOX, f_cluster=FC, **(PLT if args.plt else {}))
        m, phi = wave(n)
        g_q, g_v = field_adj_ref.plane_wave_cotangent(n, m, phi, 2, 1.0, cv=None if lean else 0, Bv=0.5, xp=torch, device="cuda",
                                                      dtype=torch.float32 if lean else torch.float64)
        out = torch.empty((n, n, n), dtype=torch.float64, device="cuda")
        walls = []
        for rep in range(REPS + 1):  # the first call warms up (code objects, the allocator)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            zd.field_vjp(p, ps, g_q=g_q, g_v=g_v, eig=eig, out=out)
            torch.cuda.synchronize()
            walls.append(time.perf_counter() - t0)
        rec = dict(ppd=n, variant="PLT + rescale" if args.plt else "ZA", cotangents="float32 g_q on the device" if lean else "float64 g_q and g_v on the device",
                   field_vjp_wall_s=min(walls[1:]), calls_traced=REPS + 1)
        if not args.plt:  # the closed form (ZA on a density field)
            sites = np.random.default_rng(n).integers(0, n, (64, 3))
            idx = torch.from_numpy(sites).cuda()
            got = out[idx[:, 0], idx[:, 1], idx[:, 2]].cpu().numpy()
            want = field_adj_ref.plane_wave_adjoint(n, m, phi, 2, 1.0, BOX, sites, cv=None if lean else 0, Bv=0.5, f_cluster=FC)
            rec["closed_form_error_over_amplitude"] = float(np.abs(got - want).max() / np.abs(want).max())
        del g_q, g_v, out
        torch.cuda.empty_cache()
        if not args.traced:  # the forward field run it differentiates, same size, NULL sink
            a = torch.zeros((n, n, n), dtype=torch.float64, device="cuda")
            a[1, 2, 3] = 1.0
            fw = [zd.generate_field(p, ps, a, eig=eig, collect=False)["seconds_total"] for _ in range(2)]
            rec["generate_field_passes_s"] = min(fw)
            del a
            torch.cuda.empty_cache()
        print("RESULT " + json.dumps(rec), flush=True)


def run_worker(args, plt, traced, tag):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--sizes", ",".join(str(s) for s in args.sizes)] + (["--plt"] if plt else []) \
        + (["--traced"] if traced else [])
    tdir = tempfile.mkdtemp(prefix="field_vjp_trace_%s_" % tag) if traced else None  # (the trace is read below and not kept)
    if traced:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tdir, "--"] + cmd
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=420)  # (a worker that hangs ends the script)
    if r.returncode:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit("worker failed (%s)" % tag)
    recs = [json.loads(ln[7:]) for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    kern = {}
    if traced:
        for f in glob.glob(os.path.join(tdir, "**", "*kernel_trace.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                name = row["Kernel_Name"]
                if "k_fadj_" not in name and "k_field_y" not in name:
                    continue
                stage = name.split("k_")[1].split("<")[0]
                n = int(name.split("<")[1].split(",")[0])
                kern.setdefault(n, {}).setdefault("k_" + stage, 0.0)
                kern[n]["k_" + stage] += (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-6
        shutil.rmtree(tdir, ignore_errors=True)
    return recs, kern


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512,1024,2048")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_vjp_times.jsonl"))
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--plt", action="store_true")
    ap.add_argument("--traced", action="store_true")
    args = ap.parse_args()
    args.sizes = [int(s) for s in args.sizes.split(",")]
    if args.worker:
        return worker(args)
    intake = {}
    for ln in open(os.path.join(ROOT, "profiles", "field_intake_times.jsonl")):
        d = json.loads(ln)
        if "intake_kernels_ms" in d:
            intake[d["ppd"]] = d["intake_kernels_ms"]
    lines = [dict(what="adjoint of a field run (zd_kernels_field_adj.hip), api.field_vjp with cotangents and result on the device, one MI355X; "
                       "kernel times: rocprofv3 --kernel-trace, a run of its own per variant, mean over %d calls (the first one included: kernel "
                       "time does not depend on it); wall = host clock around a call that ends in a device synchronise, best of %d after a "
                       "warm-up, profiler off; bytes by count from the shapes; generate_field_passes_s = zd_stats.seconds_total of the forward "
                       "field run at the same size (NULL sink, best of 2), same process" % (REPS + 1, REPS))]
    for plt in (False, True):
        tag = "plt" if plt else "za"
        plain, _ = run_worker(args, plt, False, tag)
        traced, kern = run_worker(args, plt, True, tag)
        for rec in plain:
            n = rec["ppd"]
            lean = n >= 2048
            bpp, npass = bytes_per_point(plt, not lean, 4 if lean else 8)
            k = {s: v / rec["calls_traced"] for s, v in sorted(kern.get(n, {}).items())}
            total = sum(k.values())
            rec.pop("calls_traced")
            rec.update(source="rocprofv3 --kernel-trace", forward_passes=npass, **{s + "_ms": round(v, 3) for s, v in k.items()})
            rec.update(adjoint_kernels_ms=round(total, 3), bytes_per_point=bpp, bytes_by_count=float(bpp) * n ** 3)
            if total > 0:
                rec.update(TBps=round(bpp * n ** 3 / (total * 1e-3) / 1e12, 2), fraction_of_8TBps_peak=round(bpp * n ** 3 / (total * 1e-3) / 8e12, 3),
                           ratio_to_generate_field_passes=round(total * 1e-3 / rec["generate_field_passes_s"], 2))
                if n in intake:
                    rec.update(intake_kernels_ms=intake[n], ratio_to_intake_kernels=round(total / intake[n], 2))
            lines.append(rec)
    with open(args.out, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")
            print(json.dumps(ln))


if __name__ == "__main__":
    main()
