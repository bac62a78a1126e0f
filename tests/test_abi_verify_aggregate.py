"""dg16_groth16_verify_aggregate is part of the ABI at every layer (no GPU needed): libdg16.so exports it, the Python
binding lists it with a signature, and verify.PreparedVerifyingKey has the method that calls it."""

import ctypes
import inspect

import numpy as np

SYMBOL = "dg16_groth16_verify_aggregate"


def test_symbol_is_exported_and_listed():
    import dg16_amd  # noqa: F401
    from dg16_amd.lib import load, EXPORTED
    L = load()
    assert SYMBOL in EXPORTED
    assert hasattr(L, SYMBOL), "libdg16.so does not export %s" % SYMBOL
    fn = getattr(L, SYMBOL)
    # ctx, vk, inputs, n_public, proofs, n_proofs, coeffs, flags, accepted, channel
    assert fn.argtypes == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                           ctypes.c_size_t, ctypes.c_void_p, ctypes.c_uint, ctypes.c_void_p, ctypes.c_int]


def test_method_exists_with_the_documented_parameters():
    import dg16_amd  # noqa: F401
    from dg16_amd import verify
    sig = inspect.signature(verify.PreparedVerifyingKey.verify_aggregate)
    assert list(sig.parameters) == ["self", "public_inputs", "proofs", "coeffs", "scalars_mont", "device", "channel",
                                    "n_proofs"]
    assert sig.parameters["coeffs"].default is None and sig.parameters["device"].default is False


def test_drawn_coefficients_are_nonzero_128_bit_values():
    import dg16_amd  # noqa: F401
    from dg16_amd import verify
    c = verify.random_coefficients(300)
    assert c.shape == (300, 2) and c.dtype == np.uint64
    assert (c != 0).any(axis=1).all()
    assert len({bytes(row) for row in c}) == 300
    assert verify.random_coefficients(0).shape == (0, 2)
