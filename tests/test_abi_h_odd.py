"""DG16_F_H_ODD is one flag of the existing dg16_ext_wit_h, not a new entry point: include/dg16.h, the Python binding and
the dg16-sys crate agree that it is 256, that it collides with no other flag, and that ext_wit::h has the one symbol it
had; the Python and Rust surfaces expose it with the mirror as the default."""

import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def _header_flags():
    body = re.search(r"enum dg16_flags \{(.*?)\};", _read("include", "dg16.h"), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return {k: int(v) for k, v in re.findall(r"(DG16_F_[A-Z_]+)\s*=\s*(\d+)u", body)}


def test_the_flag_is_256_everywhere():
    from dg16_amd import lib
    flags = _header_flags()
    assert flags["DG16_F_H_ODD"] == 256
    assert [k for k, v in flags.items() if v & 256] == ["DG16_F_H_ODD"]
    assert lib.F_H_ODD == 256
    rust = _read("bindings", "dg16-sys", "src", "lib.rs")
    assert re.findall(r"pub const DG16_F_H_ODD: c_uint = (\d+);", rust) == ["256"]


def test_no_symbol_was_added():
    from dg16_amd.lib import EXPORTED
    hdr = re.sub(r"/\*.*?\*/", "", _read("include", "dg16.h"), flags=re.S)
    declared = set(re.findall(r"\b(dg16_[a-z0-9_]+)\s*\(", hdr))
    assert [s for s in sorted(declared) if "ext_wit" in s or "odd" in s] == ["dg16_ext_wit_h"]
    assert [s for s in EXPORTED if "ext_wit" in s or "odd" in s] == ["dg16_ext_wit_h"]
    rust = _read("bindings", "dg16-sys", "src", "lib.rs")
    fns = re.findall(r"pub fn (dg16_[a-z0-9_]+)\s*\(", rust)
    assert [s for s in fns if "ext_wit" in s or "odd" in s] == ["dg16_ext_wit_h"]
    # the declaration itself is the one it was: nine parameters, flags last
    decl = re.search(r"int dg16_ext_wit_h\((.*?)\);", hdr, flags=re.S).group(1)
    assert len(decl.split(",")) == 9 and decl.split(",")[-1].split() == ["unsigned", "flags"]


def test_the_python_and_rust_surfaces():
    from dg16_amd import dist, groth16_mpc
    sig = inspect.signature(dist.ext_wit_h)
    assert list(sig.parameters) == ["ctx", "pp", "net", "a_share", "b_share", "c_share", "log_m", "odd"]
    assert sig.parameters["odd"].default is False
    sig = inspect.signature(groth16_mpc.party_prove)
    assert list(sig.parameters)[-1] == "h_odd" and sig.parameters["h_odd"].default is False
    shim = _read("bindings", "dg16-shim", "src", "net.rs")
    # the existing wrapper keeps its signature (bindings/patches call it); the flagged call is a sibling
    args = r"\(a: &\[F\], b: &\[F\], c: &\[F\], log_m: u32, pp: &Pss, net: \*const sys::Dg16Net\)"
    assert re.search(r"pub fn ext_wit_h<F: PrimeField>" + args, shim)
    assert re.search(r"pub fn ext_wit_h_odd<F: PrimeField>" + args, shim)
    assert "sys::DG16_F_H_ODD" in shim
