"""Times of a second-order run on a caller-supplied field (api.generate_field(order=2), csrc/zd_kernels_lpt2_field.hip) on one MI355X ->
profiles/field_lpt2_times.jsonl.

    python scripts/field_lpt2_times.py [--sizes 256,512,1024] [--out profiles/field_lpt2_times.jsonl]

Per size: a float64 white-noise density on the device, NULL sink.  zd_stats.seconds_total (the passes) and the host clock around the whole
call (intake and second-order round included) of generate_field(order=2); beside them, same commit and process, the seeded
generate(q2LPT=1) and generate_field(order=1).  The kernel time of k_gen_lpt2_field<2> / <7> against k_gen_lpt2<2> / <7> comes from a
`rocprofv3 --kernel-trace --stats` run of its own per size (a fresh child process: this file with --worker --traced), one call of each
job.  Next to the generator times go the bytes by count — a gradient pass reads 8 N^3 bytes of PhiK and writes 16 N^3 of folded inputs,
four of them per run; the final pass reads 16 N^3 (D and S) and writes the inputs of the four arrays, 7 x 8 N^3 — and the share of the
8 TB/s peak."""
import argparse
import csv
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BOX = 720.0
REPS = 2


def worker(args):
    import torch
    import zeldovich_plt_amd.api as zd
    ps = zd.PowerSpectrum.from_file(os.path.join(ROOT, "tests", "golden", "wmap1new.pow"), BOX, Pk_sigma=0.42)
    for n in args.sizes:
        gen = torch.Generator(device="cuda")
        gen.manual_seed(n)
        field = torch.randn((n, n, n), dtype=torch.float64, device="cuda", generator=gen)
        p = zd.make_params(n, boxsize=BOX)
        jobs = {"field_order2": lambda: zd.generate_field(p, ps, field, collect=False, order=2),
                "seeded_q2LPT": lambda: zd.generate(zd.make_params(n, boxsize=BOX, q2LPT=1), ps, collect=False),
                "field_order1": lambda: zd.generate_field(p, ps, field, collect=False)}
        rec = dict(ppd=n)
        for name, job in jobs.items():
            best_pass, best_wall, R = None, None, 0
            for _rep in range(1 if args.traced else REPS + 1):  # (untraced: the first call warms up)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                st = job()
                torch.cuda.synchronize()
                wall = time.perf_counter() - t0
                if args.traced or _rep > 0:
                    best_pass = st["seconds_total"] if best_pass is None else min(best_pass, st["seconds_total"])
                    best_wall = wall if best_wall is None else min(best_wall, wall)
                R = st["stream_factor"]
            rec[name + "_passes_s"], rec[name + "_wall_s"], rec[name + "_stream_factor"] = best_pass, best_wall, R
        del field
        torch.cuda.empty_cache()
        print("RESULT " + json.dumps(rec), flush=True)


def run_worker(n, traced):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--sizes", str(n)] + (["--traced"] if traced else [])
    tdir = tempfile.mkdtemp(prefix="field_lpt2_trace_%d_" % n) if traced else None  # (the trace is read below and not kept)
    if traced:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tdir, "--"] + cmd
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=300)  # (a worker that hangs ends the script)
    if r.returncode:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit("worker failed (PPD %d%s)" % (n, ", traced" if traced else ""))
    recs = [json.loads(ln[7:]) for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    kern = {}
    if traced:
        for f in glob.glob(os.path.join(tdir, "**", "*kernel_trace.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                m = re.search(r"k_gen_lpt2(_field)?<(\d+)", row["Kernel_Name"])
                if not m:
                    continue
                key = "k_gen_lpt2%s<%s>" % (m.group(1) or "", m.group(2))
                ms, cnt = kern.get(key, (0.0, 0))
                kern[key] = (ms + (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-6, cnt + 1)
        shutil.rmtree(tdir, ignore_errors=True)
    return recs[0], kern


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,512,1024")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_lpt2_times.jsonl"))
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--traced", action="store_true")
    args = ap.parse_args()
    args.sizes = [int(s) for s in args.sizes.split(",")]
    if args.worker:
        return worker(args)
    lines = [dict(what="second order on a caller-supplied field (zd_kernels_lpt2_field.hip): api.generate_field(order=2) with a float64 density on the "
                       "device, NULL sink, one MI355X, beside the seeded generate(q2LPT=1) and generate_field(order=1) of the same size and commit; "
                       "_passes_s = zd_stats.seconds_total (the passes after the plan exists), _wall_s = host clock around the call, device "
                       "synchronised (intake, second-order round and plan included), best of %d after a warm-up, profiler off; generator kernel "
                       "times: rocprofv3 --kernel-trace --stats, a run of its own per size, ONE call of each job (the sum over its launches); "
                       "bytes by count from the shapes" % REPS)]
    for n in args.sizes:
        rec, _ = run_worker(n, False)
        _traced, kern = run_worker(n, True)
        n3 = float(n) ** 3
        by_count = {"k_gen_lpt2_field<2>": 4 * (8 + 16) * n3, "k_gen_lpt2_field<7>": (16 + 7 * 8) * n3}
        for key, (ms, cnt) in sorted(kern.items()):
            rec[key + "_ms"], rec[key + "_launches"] = round(ms, 3), cnt
            if key in by_count and ms > 0:
                rec[key + "_bytes_by_count"] = by_count[key]
                rec[key + "_TBps"] = round(by_count[key] / (ms * 1e-3) / 1e12, 2)
                rec[key + "_fraction_of_8TBps_peak"] = round(by_count[key] / (ms * 1e-3) / 8e12, 3)
        for nj in ("2", "7"):
            a, b = kern.get("k_gen_lpt2_field<%s>" % nj), kern.get("k_gen_lpt2<%s>" % nj)
            if a and b and b[0] > 0:
                rec["field_over_seeded_generator_<%s>" % nj] = round(a[0] / b[0], 3)
        rec["source"] = "rocprofv3 --kernel-trace --stats"
        lines.append(rec)
    with open(args.out, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")
            print(json.dumps(ln))


if __name__ == "__main__":
    main()
