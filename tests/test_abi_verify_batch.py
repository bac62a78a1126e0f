"""libdg16.so exports the batch verifier's entry points (no GPU needed to load the library and look)."""

import ctypes


def test_batch_verifier_symbols_are_exported():
    import dg16_amd  # noqa: F401
    from dg16_amd.lib import load, lib_path, EXPORTED
    load()
    raw = ctypes.CDLL(lib_path())
    for s in ("dg16_vk_create", "dg16_vk_destroy", "dg16_groth16_verify_batch"):
        assert s in EXPORTED
        assert getattr(raw, s) is not None


def test_prepared_verifying_key_is_exported_from_the_package():
    import dg16_amd
    from dg16_amd import verify
    assert dg16_amd.PreparedVerifyingKey is verify.PreparedVerifyingKey
    for name in ("verify_batch", "close", "from_zkey", "from_parameters"):
        assert callable(getattr(verify.PreparedVerifyingKey, name))
