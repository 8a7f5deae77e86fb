"""CPU: tests/field_lpt2_ref.py — the yardstick of the GPU tests of generate_field(order=2) — is a composition of field_ref.displace and
lpt2_ref.second_order.  The two restatements carry an alive mask each; here they are held to be the same array, and the second-order
term of the fields the GPU tests use is shown to be large enough to test (>= 5 % of the first order, as tests/test_gpu_lpt2.py asks of
its own reference).  No library call.  Every test prints its figures before it asserts."""
import numpy as np
import pytest

import field_lpt2_ref
import field_ref
import lpt2_ref

BOX = 720.0
_NOISE = {}


def _noise(n):
    if n not in _NOISE:
        a = np.random.default_rng(1).standard_normal((n, n, n))
        a.setflags(write=False)
        _NOISE[n] = a
    return _NOISE[n]


@pytest.mark.parametrize("k_cutoff", [1.0, 2.0])
@pytest.mark.parametrize("n", [32, 64, 128])
def test_the_two_alive_masks_are_one(oracle, n, k_cutoff):
    p = oracle.make_params(n, boxsize=BOX, k_cutoff=k_cutoff)
    a, b = field_ref.alive_mask(p), lpt2_ref.alive_mask(n, BOX, k_cutoff)
    print("PPD", n, "k_cutoff", k_cutoff, "alive:", int(a.sum()), int(b.sum()))
    assert a.dtype == b.dtype == np.bool_ and a.sum() > 0 and np.array_equal(a, b)


@pytest.mark.parametrize("n,k_cutoff,amp", [(32, 1.0, 1.0), (64, 1.0, 1.0), (128, 1.0, 1.0), (64, 2.0, 2.0), (128, 2.0, 2.0)])
def test_the_second_order_of_the_test_fields_is_large_enough(oracle, n, k_cutoff, amp):
    """white noise as a density (2 x it at k_cutoff = 2: the ratio is linear in the amplitude) at gamma = 3/7"""
    p = oracle.make_params(n, boxsize=BOX, k_cutoff=k_cutoff)
    q, psi2 = field_lpt2_ref.first_and_unit_second(amp * _noise(n), p, BOX)
    ratio = (3.0 / 7.0) * np.abs(psi2).max() / np.abs(q).max()
    print("PPD", n, "k_cutoff", k_cutoff, "amplitude", amp, "max|psi2| / max|psi1| =", ratio)
    assert ratio >= 0.05


def test_coefficients_and_composition(oracle):
    """the defaults of a background, given coefficients, and expected() = q + gamma psi2 | alpha q + f2 gamma psi2"""
    n = 32
    p = oracle.make_params(n, boxsize=BOX, f_cluster=0.9)
    alpha, gamma, f2 = field_lpt2_ref.coefficients(p)
    a0, r0, f0 = lpt2_ref.default_coefficients(0.9)
    print("f_cluster 0.9: alpha", alpha, "gamma", gamma, "f2", f2)
    assert (alpha, gamma, f2) == (a0, -r0, f0)

    class Given:
        f_cluster, lpt2_ratio, lpt2_f2 = 0.9, -0.5, 1.7
    assert field_lpt2_ref.coefficients(Given) == (a0, 0.5, 1.7)
    q, psi2 = field_lpt2_ref.first_and_unit_second(_noise(n), p, BOX)
    d, v = field_lpt2_ref.expected(_noise(n), p, BOX)
    assert np.array_equal(d, q + gamma * psi2) and np.array_equal(v, alpha * q + f2 * gamma * psi2)


def test_one_plane_wave_has_no_second_order(oracle):
    n = 32
    p = oracle.make_params(n, boxsize=BOX)
    field = field_ref.plane_waves(n, [((3, 5, -2), 1.0, 0.4)], BOX, [(0, 0, 0)])[0]
    q, psi2 = field_lpt2_ref.first_and_unit_second(field, p, BOX)
    print("one wave: max|psi2| / max|q| =", np.abs(psi2).max() / np.abs(q).max())
    assert np.abs(q).max() > 0 and np.abs(psi2).max() <= 1e-12 * np.abs(q).max()
