"""CPU: the BLS12-377 instantiation of the resident prover is in the build and in the dispatch of csrc/prover.hip --
what can be checked without a GPU.  The proofs themselves are tests/test_gpu_prover_bls12_377.py."""

import ctypes
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import resource_report  # noqa: E402

REP = {resource_report.short(k): v for k, v in resource_report.load().items()}


def test_results_bytes_by_curve_id():
    """A record is six G1 and one G2 Jacobian points: BLS12-377 has BLS12-381's limb counts, so the same size; an id
    outside {0, 1, 2} has no record."""
    import dg16_amd  # noqa: F401
    from dg16_amd.lib import load
    L = load()
    rb = L.dg16_groth16_results_bytes
    assert rb(0) == 6 * 3 * 32 + 3 * 64
    assert rb(1) == 6 * 3 * 48 + 3 * 96
    assert rb(2) != 0 and rb(2) == rb(1)
    for curve in (3, 4, 17, -1, -2**31, 2**31 - 1):
        assert rb(curve) == 0, curve


def test_pk_create_without_a_context_leaves_no_key():
    import dg16_amd  # noqa: F401
    from dg16_amd.lib import load
    L = load()
    out = ctypes.c_void_p(0)
    for curve in (2, 3, -1):
        assert L.dg16_pk_create(None, curve, 4, 2, 4, None, None, None, None, None, None, 0, ctypes.byref(out)) == 3
        assert out.value is None


@pytest.mark.skipif(not REP, reason="no csrc/*.usage.txt: run `make -C distributed-groth16_amd/csrc` first")
def test_the_build_has_the_curves_prover_kernels():
    """prover_bls12_377.o: the four kernels of prover_impl.h over this curve's fields, and -- like the other 14-limb curve
    -- an assembly kernel whose chains stay in registers (test_kernel_resources.py holds every instance to that)."""
    mine = {k: v for k, v in REP.items() if v["file"] == "prover_bls12_377.usage.txt"}
    for prefix in ("prover_assemble_kernel<", "prover_stage1_g1_kernel<", "prover_stage1_g2_kernel<",
                   "prover_scalar_prep_kernel<"):
        hits = [k for k in mine if k.startswith(prefix)]
        assert len(hits) == 1, (prefix, sorted(mine))
        assert "bls12_377_f" in hits[0] and "bls12_381" not in hits[0] and "bn254" not in hits[0], hits
    (asm,) = [k for k in mine if k.startswith("prover_assemble_kernel<")]
    assert "bls12_377_fq" in asm
    (g1,) = [k for k in mine if k.startswith("prover_stage1_g1_kernel<")]
    assert "bls12_377_fq" in g1 and "bls12_377_fr" in g1
    # the accumulation, finalize, table and sort phases are not compiled a second time
    assert not [k for k in mine if k.startswith("msm_")], sorted(mine)
    twin = {k.replace("bls12_381", "bls12_377"): v for k, v in REP.items() if v["file"] == "prover_bls12_381.usage.txt"}
    assert sorted(twin) == sorted(mine)
    for k, r in mine.items():
        assert r["scratch"] <= twin[k]["scratch"] and r["lds"] == twin[k]["lds"], (k, r, twin[k])
