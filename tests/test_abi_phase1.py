"""libdg16.so exports the phase-1 entry points (no GPU needed to load the library and look); the struct mirrors and the
DG16_P1_* bits of include/dg16.h, of the Python binding and of the Rust block agree."""

import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dg16.h")
RUST_SYS = os.path.join(ROOT, "bindings", "dg16-sys", "src", "lib.rs")
SYMBOLS = ("dg16_points_mul_series", "dg16_srs_contribute", "dg16_srs_verify_contribution")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _header_bits():
    return {k: int(v) for k, v in re.findall(r"#define DG16_P1_([A-Z0-9_]+) (\d+)u", _header())}


def _c_fields(name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), _header(), flags=re.S).group(1)
    out = []
    for decl in body.split(";"):
        for nm in decl.split(","):
            if nm.strip():
                out.append(re.findall(r"\w+", nm)[-1])
    return out


def test_phase1_symbols_are_exported():
    import dg16_amd  # noqa: F401
    from dg16_amd.lib import load, lib_path, EXPORTED
    load()
    raw = ctypes.CDLL(lib_path())
    for s in SYMBOLS:
        assert s in EXPORTED
        assert getattr(raw, s) is not None


def test_the_struct_mirrors_have_the_headers_layout(tmp_path):
    """Sizes and offsets as the C compiler lays the header's structs out, against the ctypes mirrors."""
    from dg16_amd.lib import SrsPowersOut, SrsContributionReportC, SrsReportC
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dg16.h"\n'
                   "int main(void) {\n"
                   '  printf("%zu %zu %zu %zu %zu\\n", sizeof(dg16_srs_powers_out), sizeof(dg16_srs_contribution_report),\n'
                   "         offsetof(dg16_srs_contribution_report, failed), offsetof(dg16_srs_contribution_report, n_bad_points),\n"
                   "         offsetof(dg16_srs_contribution_report, after));\n"
                   "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    sizes = [int(v) for v in subprocess.check_output([exe], text=True).split()]
    R = SrsContributionReportC
    assert sizes == [ctypes.sizeof(SrsPowersOut), ctypes.sizeof(R), R.failed.offset, R.n_bad_points.offset, R.after.offset]
    assert ctypes.sizeof(SrsPowersOut) == 5 * ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(R) == 8 + ctypes.sizeof(SrsReportC) == 32
    assert [n for n, _ in SrsPowersOut._fields_] == _c_fields("dg16_srs_powers_out") == \
        ["tau_g1", "tau_g2", "alpha_tau_g1", "beta_tau_g1", "beta_g2"]
    assert [n for n, _ in R._fields_] == _c_fields("dg16_srs_contribution_report") == ["failed", "n_bad_points", "after"]
    assert dict(R._fields_)["after"] is SrsReportC


def test_the_bits_agree_in_header_python_and_rust():
    from dg16_amd import keygen
    bits = _header_bits()
    assert list(bits) == ["AFTER", "BAD_POINT", "IDENTITY", "BASE", "KEY_TAU", "KEY_ALPHA", "KEY_BETA", "LINK_TAU_G1",
                          "LINK_TAU_G2", "LINK_ALPHA", "LINK_BETA", "LINK_BETA_G2"]
    assert list(bits.values()) == [1 << j for j in range(12)]
    for name, value in bits.items():
        assert getattr(keygen.Phase1Report, name) == value, name
        assert keygen.Phase1Report.NAMES[value] == name.lower()
    rust = open(RUST_SYS).read()
    assert {n: int(v) for n, v in re.findall(r"pub const DG16_P1_([A-Z0-9_]+): u32 = (\d+);", rust)} == bits


def test_the_rust_mirrors_have_the_fields_of_the_header():
    rust = open(RUST_SYS).read()
    for cname, rname in (("dg16_srs_powers_out", "Dg16SrsPowersOut"),
                         ("dg16_srs_contribution_report", "Dg16SrsContributionReport")):
        rbody = re.search(r"#\[repr\(C\)\]\n#\[derive\([^\n]*\)\]\npub struct %s \{(.*?)\n\}" % rname, rust, flags=re.S).group(1)
        assert re.findall(r"pub (\w+):", rbody) == _c_fields(cname), cname
    assert re.search(r"pub after: Dg16SrsReport,", rust)
    shim = open(os.path.join(ROOT, "bindings", "dg16-shim", "src", "setup.rs")).read()
    for s in SYMBOLS:
        assert len(re.findall(r"pub fn %s\s*\(" % s, rust)) == 1
        assert "sys::%s(" % s in shim
    for fn in ("points_mul_series", "srs_contribute", "srs_verify_contribution"):
        assert re.search(r"pub fn %s<" % fn, shim), fn


def test_phase1_is_exported_from_the_package():
    import dg16_amd
    from dg16_amd import keygen, lib
    for name in ("contribute_powers", "verify_powers_contribution", "Phase1Report"):
        assert getattr(dg16_amd, name) is getattr(keygen, name)
    for name in ("points_mul_series", "srs_contribute", "srs_verify_contribution"):
        assert callable(getattr(lib.Context, name))
    rep = keygen.Phase1Report(1 | 16 | 2048, 0, (4, 0, 0, 0))
    assert not rep.accepted and rep.reasons == ["after", "key_tau", "link_beta_g2"]
    assert rep.key_tau and rep.link_beta_g2 and not rep.base and rep.after.reasons == ["tau_g1"]
    assert keygen.Phase1Report(0).accepted and keygen.Phase1Report(0).after.accepted
    rep = keygen.Phase1Report(2, 3)
    assert rep.bad_point and rep.n_bad_points == 3 and not rep.accepted
