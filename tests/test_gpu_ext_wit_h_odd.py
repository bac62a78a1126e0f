"""dg16_ext_wit_h with DG16_F_H_ODD: every party's output, byte for byte, is its row of
transpose(pack_vec(witness_map_from_abc(a, b, c, dom), pp)) -- the packed sharing of CircomReduction's witness map -- at
every packing factor, l = 1, 2, 4, 8 (4, 8, 16, 32 parties; contexts of one process).  tests/test_h_odd_oracle.py holds
the restated pipeline to the same expectation on the CPU.

Sizes: m = l (one chunk per party: the two elements a lane of h_king_kernel reads are a party's whole vector, and no fft1
level runs), m = 2 l, and m = 64 (several chunks; at l = 8, 8 of them).  The king's kernel is one launch of one
workgroup at all of them: its paths differ by l, not by m.  a, b, c hold 0 and r - 1 (tests/h_odd_cases.py)."""

import numpy as np
import pytest

import dist_pool
import h_odd_cases as HC
from oracle import corc
from oracle.pyref.fields import FR

pytestmark = pytest.mark.gpu

DG16_ERR_BAD_ARG, DG16_ERR_UNSUPPORTED = 3, 7
F_DEVICE_PTRS, F_H_ODD = 2, 256


def enc(F, vals):
    return corc.ints_to_arr([F.to_mont(v) for v in vals], 4)


def run_h(curve, l, log_m, odd):
    """Every party's output of one call, as bytes-comparable arrays."""
    F = FR[curve]
    ctxs, pps, net, D = dist_pool.parties(curve, l)
    _, _, _, qs, _ = HC.case(curve, l, log_m)
    return net.simulate_network_round(
        lambda i, h: D.ext_wit_h(ctxs[i], pps[i], h, enc(F, qs[i][0]), enc(F, qs[i][1]), enc(F, qs[i][2]), log_m, odd=odd))


def expected(curve, l, log_m):
    F = FR[curve]
    return [enc(F, row) for row in HC.case(curve, l, log_m)[4]]


def assert_same_bytes(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.tobytes() == w.tobytes(), "party %d" % i


CASES = [(c, l, lm) for c in ("bn254", "bls12_377") for l in HC.LS for lm in HC.log_ms(l, 6)] + [("bls12_381", 4, 3)]


@pytest.mark.parametrize("curve,l,log_m", CASES)
def test_flagged_h_is_the_packed_witness_map(curve, l, log_m):
    got = run_h(curve, l, log_m, True)
    assert len(got) == 4 * l and all(g.shape == ((1 << log_m) // l, 4) for g in got)
    assert_same_bytes(got, expected(curve, l, log_m))


@pytest.mark.parametrize("curve", ["bn254", "bls12_377"])
@pytest.mark.parametrize("log_m", HC.log_ms(2, 6))
def test_at_l_2_flagged_equals_unflagged(curve, log_m):
    assert_same_bytes(run_h(curve, 2, log_m, True), run_h(curve, 2, log_m, False))


def test_device_pointers_give_the_host_pointer_result():
    import torch
    curve, l, log_m = "bn254", 4, 6
    F = FR[curve]
    ctxs, pps, net, D = dist_pool.parties(curve, l)
    _, _, _, qs, _ = HC.case(curve, l, log_m)
    dev = torch.device("cuda", 0)
    ins = [[torch.from_numpy(enc(F, qs[i][k]).view(np.int64)).to(dev) for k in range(3)] for i in range(4 * l)]
    outs = [torch.zeros(((1 << log_m) // l, 4), dtype=torch.int64, device=dev) for _ in range(4 * l)]
    torch.cuda.synchronize()

    def run(i, h):
        c = ctxs[i]
        c._chk(c.L.dg16_ext_wit_h(c.h, pps[i].h, h, ins[i][0].data_ptr(), ins[i][1].data_ptr(), ins[i][2].data_ptr(),
                                  log_m, outs[i].data_ptr(), F_DEVICE_PTRS | F_H_ODD))
        c.sync()

    net.simulate_network_round(run)
    torch.cuda.synchronize()
    got = [o.cpu().numpy().view(np.uint64) for o in outs]
    assert_same_bytes(got, run_h(curve, l, log_m, True))
    assert_same_bytes(got, expected(curve, l, log_m))


def codes(curve, l, log_m, share_len, odd):
    """Every party calls ext_wit_h; the status each one gets (0 = no error)."""
    import dg16_amd
    F = FR[curve]
    ctxs, pps, net, D = dist_pool.parties(curve, l)
    share = enc(F, [1] * share_len)

    def run(i, h):
        try:
            D.ext_wit_h(ctxs[i], pps[i], h, share, share, share, log_m, odd=odd)
        except dg16_amd.Dg16Error as e:
            return e.code
        return 0
    return net.simulate_network_round(run)


@pytest.mark.parametrize("l,log_m", [(4, 1), (8, 2), (2, 0)])
def test_flagged_with_m_below_l_is_bad_arg_on_every_party_and_the_net_goes_on(l, log_m):
    """Decided before any collective: nobody waits, and the same net and contexts then run a valid flagged call."""
    curve = "bn254"
    assert codes(curve, l, log_m, 1, True) == [DG16_ERR_BAD_ARG] * (4 * l)
    ok = max(1, HC.log2(l))
    assert_same_bytes(run_h(curve, l, ok, True), expected(curve, l, ok))


def test_unflagged_at_l_4_is_still_unsupported():
    assert codes("bn254", 4, 5, 8, False) == [DG16_ERR_UNSUPPORTED] * 16
    assert DG16_ERR_UNSUPPORTED == 7
