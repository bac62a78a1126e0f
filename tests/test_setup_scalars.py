"""The identity dg16_groth16_setup rests on, on the oracle alone, and the host-side argument handling of keygen.py.

  L_i(tau) = (1/m) sum_j (tau w^-i)^j: the Lagrange vector of `setup_scalars` (oracle/pyref/groth16.py:98-103, the
  closed form (tau^m - 1) w^i / (m (tau - w^i))) is the inverse NTT of [tau^j]_{j<m} -- what the device pipeline
  computes instead of a batch inversion."""

import random

import numpy as np
import pytest

from oracle.pyref.fields import FR
from oracle.pyref.poly import Domain


@pytest.mark.parametrize("curve", ["bn254", "bls12_381", "bls12_377"])
@pytest.mark.parametrize("m", [8, 64, 1024])
def test_lagrange_vector_is_the_inverse_ntt_of_the_powers_of_tau(curve, m):
    F = FR[curve]
    p = F.p
    rng = random.Random(m)
    tau = rng.randrange(2, p)
    dom = Domain(F, m)
    assert dom.size == m
    zt = (pow(tau, m, p) - 1) % p
    assert zt != 0
    closed = [zt * dom.element(i) % p * F.inv(m * (tau - dom.element(i)) % p) % p for i in range(m)]
    assert dom.ifft([pow(tau, j, p) for j in range(m)]) == closed


def _csr(rows, nv):
    ptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint32)
    col = np.array([c for r in rows for c, _ in r], dtype=np.uint32)
    coeff = np.array([[v & (2**64 - 1), 0, 0, 0] for r in rows for _, v in r], dtype=np.uint64).reshape(-1, 4)
    return ptr, col, coeff


def _system(nv=5):
    rows = [[(0, 1), (2, 3)], [(1, 2)], [(4, 7), (3, 1), (0, 2)]]
    return dict(num_constraints=3, num_inputs=2, num_vars=nv, a=_csr(rows, nv), b=_csr(rows[::-1], nv),
                c=_csr(rows, nv))


@pytest.mark.parametrize("curve", ["bn254", "bls12_381", "bls12_377"])
def test_keygen_moduli_and_drawn_trapdoor(curve):
    from dg16_amd import keygen
    r = FR[curve].p
    assert keygen.FR_MODULUS[curve] == r
    p = keygen.prepare(curve, _system())
    assert not p["trapdoor_given"] and p["trapdoor"].shape == (5, 4)
    vals = [sum(int(x) << (64 * j) for j, x in enumerate(row)) for row in p["trapdoor"]]
    assert all(0 < v < r for v in vals) and len(set(vals)) == 5
    q = keygen.prepare(curve, _system())
    assert not np.array_equal(p["trapdoor"], q["trapdoor"])           # drawn afresh each time
    assert (p["nc"], p["ni"], p["nv"], p["log_m"]) == (3, 2, 5, 3)      # D::new(3 + 2).size() = 8
    g = keygen.prepare(curve, _system(), trapdoor=(1, 2, 3, 4, r - 1))
    assert g["trapdoor_given"] and int(g["trapdoor"][0][0]) == 1


def test_keygen_rejects_bad_arguments():
    from dg16_amd import keygen
    r = FR["bn254"].p
    for td in ((1, 2, 3, 4), (0, 1, 2, 3, 4), (1, 2, 3, 4, r), (1, 2, -3, 4, 5)):
        with pytest.raises(ValueError):
            keygen.prepare("bn254", _system(), trapdoor=td)
    with pytest.raises(ValueError):
        keygen.prepare("bn255", _system())
    bad = _system(nv=4)                       # a column index 4 with four wires
    with pytest.raises(ValueError):
        keygen.prepare("bn254", bad)
    s = _system()
    ptr, col, coeff = s["a"]
    s["a"] = (ptr[::-1].copy(), col, coeff)   # decreasing row pointers
    with pytest.raises(ValueError):
        keygen.prepare("bn254", s)
    s = _system()
    s["b"] = (s["b"][0], s["b"][1][:-1], s["b"][2])
    with pytest.raises(ValueError):
        keygen.prepare("bn254", s)
    s = _system()
    s["num_inputs"] = 6
    with pytest.raises(ValueError):
        keygen.prepare("bn254", s)


def test_generate_parameters_has_no_cpu_path():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import dg16_amd
    with pytest.raises(dg16_amd.Dg16Error):
        dg16_amd.generate_parameters(None, "bn254", _system(), trapdoor=(1, 2, 3, 4, 5))


def test_window_rule_is_exported_without_a_gpu():
    """dg16_fixed_base_window_bits: floor(log2 n) - 3 clamped to 4..16 -- the GPU tests take their sizes from it."""
    from dg16_amd.lib import load
    L = load()
    assert [L.dg16_fixed_base_window_bits(n) for n in (0, 1, 255, 256, 511, 512, 2**14, 2**19 - 1, 2**19, 2**24)] == \
        [4, 4, 4, 5, 5, 6, 11, 15, 16, 16]
