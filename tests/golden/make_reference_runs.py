"""Writes tests/golden/reference_runs/<configuration>.npz from runs of the complete reference program, oracle/_ref/zeldovich_ref
(`make -C oracle ref` where the reference's sources are mounted).  Run by hand, like make_golden.py:

    python tests/golden/make_reference_runs.py [configuration ...]

The configurations, the layout of a fixture and the signed-sum weights are in tests/reference_runs.py, which the tests import
too.  A fixture that would exceed 256 KB loses kept planes, never a configuration: the planes go in the order n/2 - 1, 1, n/2,
n - 1 until it fits."""
import io
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import reference_runs as rr  # noqa: E402
from oracle import zdo  # noqa: E402

DROP_ORDER = lambda n: [n // 2 - 1, 1, n // 2, n - 1]  # noqa: E731


def run_reference(name, tmp, par=None):
    """runs the reference program on a configuration's parameter text inside `tmp`; returns (par, out dir, stderr, eig sha)"""
    par = par if par is not None else rr.par_text(name)
    out = os.path.join(tmp, "ic_out")
    _, sha = rr.write_eigenmodes(os.path.join(tmp, "eigmodes"), zdo)
    parfile = os.path.join(tmp, "run.par")
    with open(parfile, "w") as f:
        f.write(rr.fill(par, out, os.path.join(HERE, "wmap1new.pow"), os.path.join(tmp, "eigmodes")))
    r = subprocess.run([rr.REF_EXE, parfile], cwd=tmp, capture_output=True, text=True, env=dict(os.environ, OMP_NUM_THREADS="1"))
    if r.returncode:
        raise RuntimeError("%s: the reference program failed (%d)\n%s" % (name, r.returncode, r.stderr[-2000:]))
    return par, out, r.stderr, sha


def fixture_arrays(par, out, stderr, sha):
    n = rr.par_ppd(par)
    fmt = rr.par_value(par, "ICFormat")
    qd = int(rr.par_value(par, "ZD_qdensity", "0"))
    planes = rr.read_planes(out, par, zdo.RECORD_DTYPES[fmt]) if qd != 2 else {}
    dens = rr.read_density(out, par)
    zs = sorted(planes) if planes else sorted(dens)
    md, rms = rr.printed_figures(stderr)
    files = rr.list_files(out)
    a = dict(par=np.array(par), sum_z=np.array(zs, dtype=np.int64),
             sums=np.array([rr.signed_sums(z, planes[z]) for z in zs]) if planes else np.zeros((0, 0, rr.NPATTERN)),
             file_names=np.array([f for f, _ in files]), file_sizes=np.array([s for _, s in files], dtype=np.int64),
             max_disp=md if md is not None else np.zeros(0), rms_density=np.array(rms if rms is not None else np.nan),
             eig_sha256=np.array(sha if int(rr.par_value(par, "ZD_qPLT", "0")) else ""))
    if dens is not None:
        a["dens_sums"] = np.array([rr.density_signed_sums(z, dens[z]) for z in zs])
    return a, planes, dens, zs


def write_fixture(name):
    with tempfile.TemporaryDirectory() as tmp:
        a, planes, dens, zs = fixture_arrays(*run_reference(name, tmp))
        n = rr.par_ppd(str(a["par"]))
        kept = [z for z in sorted({0, 1, n // 2 - 1, n // 2, n - 1}) if z in zs] or zs[:1]
        drop = [z for z in DROP_ORDER(n) if z in kept]
        while True:
            b = dict(a, kept_z=np.array(kept, dtype=np.int64))
            for z in kept:
                if planes:
                    b["plane_%d" % z] = planes[z]
                if dens is not None:
                    b["dens_%d" % z] = dens[z]
            buf = io.BytesIO()
            np.savez_compressed(buf, **b)
            if buf.tell() <= rr.MAX_FIXTURE_BYTES or len(kept) == 1:
                break
            kept.remove(drop.pop(0))
        if buf.tell() > rr.MAX_FIXTURE_BYTES:
            raise RuntimeError("%s: one plane alone is %d bytes" % (name, buf.tell()))
        os.makedirs(rr.FIXDIR, exist_ok=True)
        with open(os.path.join(rr.FIXDIR, name + ".npz"), "wb") as f:
            f.write(buf.getvalue())
        print("%-16s n=%d kept planes %s, %d bytes" % (name, n, kept, buf.tell()))


if __name__ == "__main__":
    if not os.path.exists(rr.REF_EXE):
        sys.exit("oracle/_ref/zeldovich_ref is missing: `make -C oracle ref` where the reference is mounted")
    for name in sys.argv[1:] or rr.fixture_names():
        write_fixture(name)
