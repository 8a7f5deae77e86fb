"""CPU: tests/field_ref.py — the numpy restatement the GPU tests of generate_field compare against — held to the oracle at N = 32.
No library call."""
import numpy as np
import pytest

import field_ref
from conftest import WMAP

N, BOX = 32, 720.0
PLT = dict(qPLT=1, qPLTrescale=1, PLT_target_z=5.0, f_cluster=0.97)


@pytest.fixture(scope="module")
def za(oracle):
    """oracle ZA records of the default seed and the density they are the displacement of (shared, read-only)"""
    op = oracle.make_params(N, boxsize=BOX)
    rec = oracle.run(op, oracle.pk_from_file(WMAP, BOX))["records"]
    delta = field_ref.delta_from_za(rec, BOX)
    delta.setflags(write=False)
    return op, rec, delta


def _err(got, ref):
    return np.abs(got - ref).max() / np.abs(ref).max()


def test_displace_returns_the_oracles_za_records(za):
    op, rec, delta = za
    q, v, dens = field_ref.displace(delta, op)
    ed, ev = _err(q, rec["d"]), _err(v, rec["v"])
    print("ZA: displacement error", ed, "velocity error", ev)
    assert ed <= 1e-12 and ev <= 1e-12
    assert np.abs(dens - delta).max() <= 1e-12 * np.abs(delta).max()  # (every mode of delta is alive: the mask removes nothing)


def test_displace_returns_the_oracles_plt_records(oracle, za):
    """the same density with the oracle's synthetic eigenmodes: the PLT + rescale records of that seed"""
    _op, _rec, delta = za
    eig = oracle.synthetic_eigenmodes(128)
    op = oracle.make_params(N, boxsize=BOX, **PLT)
    rec = oracle.run(op, oracle.pk_from_file(WMAP, BOX), eig=eig, eig_ppd=eig.shape[0])["records"]
    q, v, _dens = field_ref.displace(delta, op, eig=eig, oracle=oracle)
    ed, ev = _err(q, rec["d"]), _err(v, rec["v"])
    print("PLT + rescale: displacement error", ed, "velocity error", ev)
    assert ed <= 1e-12 and ev <= 1e-12


def test_plane_waves_closed_form_meets_displace(oracle):
    op = oracle.make_params(N, boxsize=BOX, f_cluster=0.9)
    waves = [((3, 0, 2), 1.0, 0.3), ((-5, 4, -1), 0.7, 1.1), ((N // 2 - 1, 2, 3), 0.4, -0.6)]
    rng = np.random.default_rng(3)
    sites = rng.integers(0, N, (200, 3))
    field, q_ref, v_ref = field_ref.plane_waves(N, waves, BOX, sites, f_cluster=0.9)
    q, v, dens = field_ref.displace(field, op)
    at = (sites[:, 0], sites[:, 1], sites[:, 2])
    ed, ev = np.abs(q[at] - q_ref).max() / np.abs(q_ref).max(), np.abs(v[at] - v_ref).max() / np.abs(v_ref).max()
    print("plane waves: displacement error", ed, "velocity error", ev)
    assert ed <= 1e-12 and ev <= 1e-12
    assert np.abs(dens - field).max() <= 1e-12 * np.abs(field).max()


def test_zero_rule_mask():
    """the mask against the rule written out mode by mode, with a cut-off, with corner modes, and with one mode"""
    class P:
        ppd, boxsize, k_cutoff, corner_modes, qonemode, one_mode = N, BOX, 2.0, 0, 0, (0, 0, 0)
        fundamental, nyquist = 2 * np.pi / BOX, np.pi / (BOX / N)
    k = field_ref.wavenumbers(N)
    kz, ky, kx = np.meshgrid(k, k, k, indexing="ij")
    k2 = kx ** 2 + ky ** 2 + kz ** 2
    m = field_ref.alive_mask(P)
    assert not m[k2 * P.fundamental ** 2 >= (P.nyquist / 2) ** 2].any() and m[(k2 > 0) & (k2 < 64)].all() and not m[0, 0, 0]
    P.corner_modes = 1
    m = field_ref.alive_mask(P)
    cheb = np.maximum(np.maximum(np.abs(kx), np.abs(ky)), np.abs(kz))
    assert m[(cheb < 8) & (k2 > 0)].all() and not m[(np.abs(kx) == 8) | (np.abs(ky) == 8) | (np.abs(kz) == 8)].any()
    assert m[(cheb > 8) & (cheb < 16) & (np.abs(kx) != 8) & (np.abs(ky) != 8) & (np.abs(kz) != 8)].all() and not m[cheb == 16].any()
    P.corner_modes, P.k_cutoff, P.qonemode, P.one_mode = 0, 1.0, 1, (3, 2, -4)
    m = field_ref.alive_mask(P)
    assert m.sum() == 2 and m[-4, 2, 3] and m[4, -2, -3]
    P.one_mode = (3, 0, -4)  # ky = 0, kz < 0: its mirror image is the mode the path reads, and that one is not ZD_one_mode
    assert field_ref.alive_mask(P).sum() == 0
