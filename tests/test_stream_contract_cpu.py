"""The header's list of the device entries that wait for their stream, held to the table the GPU test works from: the conventions
paragraph of include/ogg_hip.h names them, tests/test_gpu_streams.py skips the no-wait observation for exactly the entries of its
WAITS table, and neither may drift from the other or from the code.  No GPU is needed: the header and the sources are read as text."""
import os
import re

import test_gpu_streams as TS
from ocean_model_grid_generator_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "ogg_hip.h")).read()
PKG = os.path.join(ROOT, "ocean_model_grid_generator_amd")


def conventions():
    """the comment at the top of the header"""
    return HEADER[:HEADER.index("#ifndef OGG_HIP_H")]


def comment_before(name):
    """the comment that ends right before the declaration of ``name``"""
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*(?:int|long) %s\(" % name, HEADER, re.S)
    assert m, "no comment right before the declaration of %s" % name
    return " ".join(m.group(1).split())


def test_the_headers_list_is_the_table():
    text = conventions()
    listed = text[text.index("The exceptions"):text.index("and the displaced-pole entries")]
    assert set(re.findall(r"ogg_\w+_dev", listed)) == set(TS.WAITS)


def test_every_listed_entry_says_so_in_its_own_comment():
    for name in TS.WAITS:
        assert "Waits for the stream" in comment_before(name), name


def test_no_other_device_entry_claims_to_wait():
    entries = {n for n in _lib.SIGNATURES if n.startswith("ogg_") and n.endswith("_dev")}
    assert set(TS.WAITS) <= entries
    for name in sorted(entries - set(TS.WAITS)):
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*(?:int|long) %s\(" % name, HEADER, re.S)
        assert not (m and "Waits for the stream" in m.group(1)), name


def test_every_reason_points_at_a_wait_in_the_code():
    """file:line of every reason: a line of the named source that waits (a table that has drifted from the code fails here)"""
    for name, reason in TS.WAITS.items():
        m = re.search(r"csrc/(\w+\.hip):(\d+)$", reason)
        assert m, (name, reason)
        lines = open(os.path.join(PKG, "csrc", m.group(1))).read().split("\n")
        assert "hipStreamSynchronize(" in lines[int(m.group(2)) - 1], (name, reason, lines[int(m.group(2)) - 1])


def test_the_exemptions_have_reasons_and_are_entries():
    entries = {n for n in _lib.SIGNATURES if n.startswith("ogg_") and n.endswith("_dev")}
    assert set(TS.NOT_OBSERVED) <= entries and all(len(r) > 20 for r in TS.NOT_OBSERVED.values())
    assert not set(TS.NOT_OBSERVED) & set(TS.WAITS)
