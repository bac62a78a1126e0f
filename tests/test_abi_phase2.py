"""libdg16.so exports the phase-2 entry points (no GPU needed to load the library and look), and the package exports
their Python surface."""

import ctypes


def test_phase2_symbols_are_exported():
    import dg16_amd  # noqa: F401
    from dg16_amd.lib import load, lib_path, EXPORTED
    load()
    raw = ctypes.CDLL(lib_path())
    for s in ("dg16_points_scale", "dg16_groth16_contribute", "dg16_groth16_verify_contribution"):
        assert s in EXPORTED
        assert getattr(raw, s) is not None


def test_the_struct_mirrors_have_the_headers_layout():
    from dg16_amd.lib import Groth16Key, Phase2ReportC
    assert ctypes.sizeof(Groth16Key) == 8 * ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(Phase2ReportC) == 24
    assert [n for n, _ in Groth16Key._fields_] == ["a_query", "b_g1_query", "b_g2_query", "h_query", "l_query",
                                                   "fixed_points", "gamma_g2", "gamma_abc_g1"]


def test_phase2_is_exported_from_the_package():
    import dg16_amd
    from dg16_amd import keygen, lib
    for name in ("contribute", "verify_contribution", "verify_parameters", "Phase2Report"):
        assert getattr(dg16_amd, name) is getattr(keygen, name)
    for name in ("points_scale", "groth16_contribute", "groth16_verify_contribution"):
        assert callable(getattr(lib.Context, name))
    rep = keygen.Phase2Report(1 | 16, 4, 7, 2)
    assert not rep.accepted and rep.reasons == ["bad_point", "l"] and rep.bad_array == "after.l_query"
    assert rep.bad_index == 7 and rep.n_bad_points == 2
    assert keygen.Phase2Report(0).accepted and keygen.Phase2Report(0).bad_array is None
