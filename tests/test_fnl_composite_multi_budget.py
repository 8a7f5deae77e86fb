"""ZD_f_NL on the composite grids on several ranks: the split of the job (zd_choose_pass_groups: host code, no GPU needed).  Per rank
the chooser counts PhiK / G, the phi round's peak (its store / G and the exchange ring) and each main pass's store / G beside PhiK, and
takes only stream factors whose z lines N / R have a composite transform and deal out over the ranks."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

GB = 1 << 30
FNL = dict(f_NL=2.0e4, n_s=0.96, Omega_M=0.31)


def _refq_lengths():
    src = open(os.path.join(ROOT, "zeldovich_plt_amd", "csrc", "zd_kernels_np2_ref.hip")).read()
    body = src[src.index("#define REFQ_SIZES(X)"):]
    body = body[:body.index("\n\n")]
    return {int(p) * int(q) for p, q, _w in re.findall(r"X\((\d+), (\d+), (\d+)\)", body)}


def _choose(n, ngpu, budget_gb, **kw):
    import zeldovich_plt_amd.api as zd
    L = zd.load_library()
    g, R = C.c_int32(0), C.c_int32(0)
    rc = L.zd_choose_pass_groups(C.byref(zd.make_params(n, **FNL, **kw)), ngpu, int(budget_gb * GB), C.byref(g), C.byref(R))
    return rc, g.value, R.value


@pytest.mark.parametrize("n,ngpu", [(3456, 8), (4000, 8), (3072, 4)])
def test_composite_fnl_fits_several_ranks(n, ngpu):
    # PPD 3456 / 8: PhiK 39 GiB + phi store 78 GiB + ring; 4000 / 8 and 3072 / 4 need R = 2 beside PhiK
    rc, g, R = _choose(n, ngpu, 272)
    assert rc == 0 and g == 1, (rc, g, R)
    assert n % R == 0 and (n // R) in _refq_lengths() and (n // R) % ngpu == 0, R


def test_composite_fnl_stream_factors():
    assert _choose(3456, 8, 272)[2] == 1
    assert _choose(4000, 8, 272)[2] == 2   # R = 1: 238 GiB of store + 60 GiB of PhiK per rank
    assert _choose(3072, 4, 272)[2] == 2   # R = 1: 216 + 54 GiB and the ring
    assert _choose(3072, 4, 150)[0] == 1   # the phi round alone (54 + 108 GiB) does not fit


def test_composite_fnl_refusals():
    assert _choose(3456, 1, 272)[0] == 1                 # one rank: PhiK alone is 8 N^3 = 308 GiB
    assert _choose(1000, 2, 272)[0] == 1                 # convolution-only PPD
    assert _choose(3456, 8, 272, pass_groups=2)[0] == 1  # f_NL runs as one group
