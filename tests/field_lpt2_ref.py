"""numpy restatement of a second-order (2LPT) run on a caller-supplied field (definition: zeldovich_plt_amd/csrc/zd_kernels_lpt2_field.hip),
for the tests of generate_field(order=2) / Plan.from_field(order=2).  It is the composition of two existing restatements and adds no
arithmetic of its own: field_ref.displace gives the first order of the field, lpt2_ref.second_order the second order of that
displacement.  tests/test_field_lpt2.py holds the two alive masks to each other.

Arrays are [z][y][x]; vector fields [z][y][x][3] in the records' order (q_z, q_y, q_x)."""
import numpy as np

import field_ref
import lpt2_ref


def coefficients(params):
    """(alpha, gamma, f2) as zd_route.h resolves them: alpha = vnorm of the f_cluster background, gamma = -lpt2_ratio, f2; a zero
    lpt2_ratio / lpt2_f2 in the parameters means that background's own"""
    alpha, ratio, f2 = lpt2_ref.default_coefficients(params.f_cluster)
    given_ratio, given_f2 = getattr(params, "lpt2_ratio", 0.0), getattr(params, "lpt2_f2", 0.0)
    return alpha, -(given_ratio if given_ratio != 0.0 else ratio), (given_f2 if given_f2 != 0.0 else f2)


def first_and_unit_second(a, params, boxsize):
    """(q, psi2 at gamma = 1) of the density field a: q the first-order displacement a field run delivers, psi2 the second-order
    displacement of q with lpt2_ratio = -1 (the caller scales it by gamma)"""
    n = int(params.ppd)
    q, _v, _dens = field_ref.displace(a, params)
    mask = lpt2_ref.alive_mask(n, boxsize, params.k_cutoff, int(getattr(params, "corner_modes", getattr(params, "CornerModes", 0))))
    return q, lpt2_ref.second_order(q, boxsize, mask, lpt2_ratio=-1.0)


def expected(a, params, boxsize):
    """(displacement, velocity) of generate_field(order=2): q + gamma psi2, alpha q + f2 gamma psi2"""
    alpha, gamma, f2 = coefficients(params)
    q, psi2 = first_and_unit_second(a, params, boxsize)
    return q + gamma * psi2, alpha * q + f2 * gamma * psi2
