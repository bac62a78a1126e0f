"""libdg16.so exports the request-packing entry points (no GPU needed to load the library and look), the struct mirrors
have the header's layout, and the package exports their Python surface."""

import ctypes
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("dg16_fr_expand", "dg16_pss_scalar_chunks", "dg16_pss_pack_scalars", "dg16_request_pack")
FIELDS = ["a", "b", "c", "a_share", "ax_share"]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dg16.h")).read(), flags=re.S)


def test_request_pack_symbols_are_exported():
    import dg16_amd  # noqa: F401
    from dg16_amd.lib import load, lib_path, EXPORTED
    load()
    raw = ctypes.CDLL(lib_path())
    for s in SYMBOLS:
        assert s in EXPORTED
        assert getattr(raw, s) is not None


def test_the_struct_mirrors_have_the_headers_layout():
    from dg16_amd.lib import RequestShares
    assert ctypes.sizeof(RequestShares) == 5 * ctypes.sizeof(ctypes.c_void_p)
    assert [n for n, _ in RequestShares._fields_] == FIELDS
    body = re.search(r"typedef struct dg16_request_shares \{(.*?)\} dg16_request_shares;", _header(), flags=re.S).group(1)
    assert re.findall(r"\*(\w+)", body) == FIELDS
    rust = open(os.path.join(ROOT, "bindings", "dg16-sys", "src", "lib.rs")).read()
    rbody = re.search(r"pub struct Dg16RequestShares \{(.*?)\n\}", rust, flags=re.S).group(1)
    assert re.findall(r"pub (\w+): \*mut c_void", rbody) == FIELDS


def test_the_layout_constants_agree():
    from dg16_amd import dist
    hdr = dict(re.findall(r"(DG16_PACK_[A-Z]+)\s*=\s*(\d+)", _header()))
    assert hdr == {"DG16_PACK_CHUNKS": "0", "DG16_PACK_DFFT": "1"}
    assert (dist.PACK_CHUNKS, dist.PACK_DFFT) == (0, 1)
    rust = open(os.path.join(ROOT, "bindings", "dg16-sys", "src", "lib.rs")).read()
    assert dict(re.findall(r"pub const (DG16_PACK_[A-Z]+): c_int = (\d+);", rust)) == hdr


def test_the_new_calls_take_no_flags_word():
    """Host pointers only: none of the new declarations admits the device-pointer flag (tests/test_stream_table.py's
    rule), so none needs a row in the stream-order table."""
    import test_stream_table as ST
    decl = ST.declarations()
    for s in SYMBOLS:
        if s == "dg16_pss_scalar_chunks":           # returns a size, not a status
            continue
        assert s in decl, s
        assert not ST.admits_device_pointers(*decl[s]), s


def test_the_python_surface():
    from dg16_amd import dist, groth16_mpc, lib
    assert callable(lib.Context.fr_expand)
    assert list(inspect.signature(lib.Context.fr_expand).parameters) == ["self", "curve", "seed", "stream", "first", "n",
                                                                         "mont"]
    pp = dist.PackedSharingParams
    assert list(inspect.signature(pp.pack_scalars).parameters) == ["self", "values", "layout", "blinds"]
    assert inspect.signature(pp.pack_scalars).parameters["blinds"].default is None
    assert list(inspect.signature(pp.pack_from_public_rand).parameters) == ["self", "secrets", "blinds"]
    sig = inspect.signature(groth16_mpc.pack_request)
    assert list(sig.parameters)[:7] == ["pp", "a", "b", "c", "assignment", "num_inputs", "seed"]
    assert sig.parameters["seed"].default is None
