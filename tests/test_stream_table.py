"""No GPU: every function of include/dg16.h that admits DG16_F_DEVICE_PTRS has an ordering test -- a row of
tests/stream_cases.py (run by tests/test_gpu_stream_order.py), one of the tests of the entry points without a channel, or
an explicit exception with its reason.  A new entry point then cannot arrive without one."""

import os
import re

import stream_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declarations():
    """name -> (parameter text, the comment block right above the declaration) for every `int dg16_*(...)` of the header."""
    text = open(os.path.join(ROOT, "include", "dg16.h")).read()
    out = {}
    for m in re.finditer(r"^int (dg16_\w+)\(([^;]*?)\);", text, re.M | re.S):
        before = text[:m.start()].rstrip()
        comment = ""
        if before.endswith("*/"):
            comment = before[before.rindex("/*"):]
        out[m.group(1)] = (" ".join(m.group(2).split()), comment)
    return out


def admits_device_pointers(params, comment):
    """The signature: a context and a `flags` word (DG16_F_DEVICE_PTRS is a flag, and only a context has a GPU); or the
    declaration's own comment names the flag."""
    return ("dg16_ctx *ctx" in params and "unsigned flags" in params) or \
        ("DG16_F_DEVICE_PTRS" in comment and "dg16_ctx *ctx" in params)


def test_the_header_parses():
    decl = declarations()
    assert len(decl) >= 70, sorted(decl)          # the header declares 70 status-returning functions today
    for name in ("dg16_msm", "dg16_groth16_prove", "dg16_set_stream", "dg16_groth16_setup_srs", "dg16_wire_fr_decode"):
        assert name in decl, name
    # host-only calls are not in scope
    assert not admits_device_pointers(*decl["dg16_groth16_verify"])
    assert not admits_device_pointers(*decl["dg16_proof_compress"])
    assert not admits_device_pointers(*decl["dg16_set_stream"])
    assert admits_device_pointers(*decl["dg16_vk_create"]) and admits_device_pointers(*decl["dg16_pk_create"])


def test_every_device_pointer_entry_point_has_an_ordering_test_or_a_reason():
    decl = declarations()
    admitted = {n for n, d in decl.items() if admits_device_pointers(*d)}
    covered = SC.covered_entry_points()
    missing = sorted(admitted - covered - set(SC.EXCEPTIONS))
    assert not missing, "no row in tests/stream_cases.py and no exception for: %s" % ", ".join(missing)
    # the lists stay honest: nothing is both tested and excused, nothing names a function the header does not have
    assert not covered & set(SC.EXCEPTIONS), sorted(covered & set(SC.EXCEPTIONS))
    assert not (covered | set(SC.EXCEPTIONS)) - admitted, sorted((covered | set(SC.EXCEPTIONS)) - admitted)
    for name, reason in SC.EXCEPTIONS.items():
        assert len(reason.split()) >= 4, "%s: an exception carries a reason" % name


def test_the_table_is_well_formed():
    names = [r.name for r in SC.ROWS]
    assert len(names) == len(set(names))
    for r in SC.ROWS:
        assert r.entries and r.channels in ((0,), (0, 1, 2)), r.name
        assert all(h in SC.HOST_POINTERS for h in r.host), r.name
    # the calls that use all three channels, or have none to choose, run with the caller's stream on channel 0 only
    for r in SC.ROWS:
        if set(r.entries) & {"dg16_groth16_prove", "dg16_groth16_msms", "dg16_groth16_msms_h", "dg16_groth16_assemble", "dg16_bases_upload"}:
            assert r.channels == (0,), r.name
    # the tests the table points to exist
    src = open(os.path.join(ROOT, "tests", "test_gpu_stream_order.py")).read()
    for fn, test in SC.NO_CHANNEL.items():
        assert "def %s(" % test in src, (fn, test)
