"""The QAP kernels' guard against untrusted CSR indices (qap_kernel in csrc/field_ops.hip, qap_r1cs_kernel in
csrc/qap_libsnark.hip), which only the device-pointer entry points reach -- the host-pointer ones validate before the
launch.  A lane that meets a column >= num_vars, a decreasing row_ptr or a row longer than num_vars zeroes its row and
raises the context's sticky flag; the call returns DG16_OK, the next dg16_sync returns DG16_ERR_BAD_ARG once, and every
other row is what the oracle computes.

Each run takes a synthetic system of 300 constraints (two workgroups) on the device and a copy with ONE defect.  The
expected vectors are the oracle's (corc.qap; the big-int model of tests/test_libsnark_model.py for the form with a C
matrix) on the rows as the arrays describe them with the defective row emptied: a lowered row_ptr[i + 1] is also where
row i + 1 starts, so that row legitimately sums other entries than before.

Deliberately not covered: a row_ptr beyond the column / coefficient arrays.  The kernels do not know the arrays' lengths
and say so; such a case would read outside an allocation.  Every row_ptr here stays inside the arrays."""

import numpy as np
import pytest

from oracle import corc
from oracle.pyref.fields import FR
from oracle.pyref import groth16 as G
from gpu_util import ctx
from test_gpu_prover import enc_fr
from test_gpu_setup import csr_of
import test_libsnark_model as M

pytestmark = pytest.mark.gpu

NC, NI, NW = 300, 3, 60
NV = NI + NW
LOG_M = 9
FORMS = ["qap", "qap_rows", "qap_r1cs"]


def _flat(rows):
    """rows of (coefficient, column) -> row_ptr, col, coefficient lists."""
    ptr, col, cf = [0], [], []
    for row in rows:
        cf += [c for c, _ in row]
        col += [i for _, i in row]
        ptr.append(len(col))
    return [ptr, col, cf]


def _defect(kind, mats):
    """Applies one defect in place; returns the row it spoils.  mats: [ptr, col, cf] of A, B, C."""
    if kind == "col_eq_nv_a_row0":
        ptr, col, _ = mats[0]
        col[ptr[0]] = NV
        return 0
    if kind == "col_eq_nv_b_last_row":
        ptr, col, _ = mats[1]
        col[ptr[NC] - 1] = NV
        return NC - 1
    if kind == "col_all_ones":
        ptr, col, _ = mats[0]
        col[ptr[257] + 1] = 0xFFFFFFFF
        return 257
    if kind == "row_ptr_decreases":
        ptr = mats[0][0]
        assert ptr[100] >= 1
        ptr[101] = ptr[100] - 1
        return 100
    if kind == "row_longer_than_nv":
        ptr, col, cf = mats[1]
        extra = NV + 1 - (ptr[201] - ptr[200])
        at = ptr[201]
        col[at:at] = [k % NV for k in range(extra)]
        cf[at:at] = [k + 2 for k in range(extra)]
        for j in range(201, NC + 1):
            ptr[j] += extra
        assert ptr[201] - ptr[200] == NV + 1 and max(col) < NV
        return 200
    raise KeyError(kind)


DEFECTS = ["col_eq_nv_a_row0", "col_eq_nv_b_last_row", "col_all_ones", "row_ptr_decreases", "row_longer_than_nv"]


def _rows_as_described(mat):
    """The rows the arrays describe, and the set of rows the guard must refuse (emptied here)."""
    ptr, col, cf = mat
    rows, bad = [], set()
    for j in range(NC):
        lo, hi = ptr[j], ptr[j + 1]
        assert 0 <= lo <= len(col) and 0 <= hi <= len(col)                     # never outside the arrays
        if hi < lo or hi - lo > NV or any(c >= NV for c in col[lo:hi]):
            bad.add(j)
            rows.append([])
        else:
            rows.append(list(zip(cf[lo:hi], col[lo:hi])))
    return rows, bad


def _csr_arrays(F, mat):
    ptr, col, cf = mat
    return (np.asarray(ptr, dtype=np.uint32), np.asarray(col, dtype=np.uint32), enc_fr(F, cf).reshape(-1, 4))


def _oracle(curve, F, mats, w, with_c):
    """(a, b, c) Montgomery arrays [m][4] with the refused rows zeroed, and the refused rows."""
    m = 1 << LOG_M
    desc = [_rows_as_described(mat) for mat in (mats if with_c else mats[:2])]
    bad = set().union(*[b for _, b in desc])
    if with_c:
        r1cs = dict(num_instance=NI, num_witness=NW, num_constraints=NC, a=desc[0][0], b=desc[1][0], c=desc[2][0])
        a, b, c, dom = M.libsnark_abc(r1cs, w, F)
        assert dom.size == m
        out = [enc_fr(F, v) for v in (a, b, c)]
    else:
        out = corc.qap(curve, NC, NI, m, csr_of(F, desc[0][0]), csr_of(F, desc[1][0]), enc_fr(F, w))
    for v in out:
        v[sorted(bad)] = 0
    return out, bad


def _run(curve, form, mats, w_dev, row_start):
    """One call on device pointers with 0xAB-filled outputs: the three output arrays.  The call itself must succeed."""
    import torch
    dev = torch.device("cuda", 0)
    F = FR[curve]
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(dev)      # noqa: E731
    d = [up(x) for mat in mats for x in _csr_arrays(F, mat)]
    m = 1 << LOG_M
    rows = m // 2 if form == "qap_rows" else m
    out = [torch.full((rows * 32,), 0xAB, dtype=torch.uint8, device=dev) for _ in range(3)]
    torch.cuda.synchronize()
    p = [t.data_ptr() for t in d]
    o = [t.data_ptr() for t in out]
    c = ctx()
    if form == "qap":
        c.qap_dev(curve, NC, NI, NV, LOG_M, *p[:6], w_dev.data_ptr(), *o)
    elif form == "qap_rows":
        c.qap_rows_dev(curve, NC, NI, NV, LOG_M, *p[:6], w_dev.data_ptr(), row_start, 2, *o)
    else:
        c.qap_r1cs_dev(curve, NC, NI, NV, LOG_M, p, w_dev.data_ptr(), *o)
    return out, d


def _host(out):
    return [t.cpu().numpy().view(np.uint64).reshape(-1, 4) for t in out]


@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind", DEFECTS)
def test_one_defect_zeroes_its_row_and_raises_the_flag_once(curve, form, kind):
    import torch
    import dg16_amd
    F = FR[curve]
    r1cs, w = G.synthetic_r1cs(F, num_constraints=NC, num_instance=NI, num_witness=NW, seed=8, nnz=4)
    assert len(w) == NV
    with_c = form == "qap_r1cs"
    clean = [_flat(r1cs[k]) for k in "abc"]
    broken = [[list(x) for x in mat] for mat in clean]
    bad_row = _defect(kind, broken)
    want_clean, none = _oracle(curve, F, clean, w, with_c)
    want, bad = _oracle(curve, F, broken, w, with_c)
    assert not none and bad == {bad_row}
    if kind != "row_ptr_decreases":                  # every other defect leaves every other row as it was
        keep = np.ones(1 << LOG_M, dtype=bool)
        keep[bad_row] = False
        assert all(np.array_equal(x[keep], y[keep]) for x, y in zip(want, want_clean))
    assert all(v[bad_row].any() for v in want_clean[:2])          # the row is worth zeroing
    row_start = bad_row % 2
    sl = slice(row_start, None, 2) if form == "qap_rows" else slice(None)
    c = ctx()
    w_dev = torch.from_numpy(enc_fr(F, w).view(np.uint8).reshape(-1).copy()).to(torch.device("cuda", 0))
    c.sync(0)
    try:
        out, alive = _run(curve, form, broken, w_dev, row_start)          # returns DG16_OK: no exception
        with pytest.raises(dg16_amd.Dg16Error, match="coefficient out of range") as e:
            c.sync(0)
        assert e.value.code == 3                                            # DG16_ERR_BAD_ARG
        got = _host(out)
        slot = bad_row // 2 if form == "qap_rows" else bad_row
        for g, x in zip(got, want):
            assert not g[slot].any()
            assert np.array_equal(g, x[sl])
        c.sync(0)                                                           # the flag was cleared: clean
        out, alive = _run(curve, form, clean, w_dev, row_start)
        c.sync(0)
        for g, x in zip(_host(out), want_clean):
            assert np.array_equal(g, x[sl])
    finally:
        try:                                                                # never leave the sticky flag to a later test
            c.sync(0)
        except dg16_amd.Dg16Error:
            pass
