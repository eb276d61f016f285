"""CPU, no library: every helper that the point-cloud sources share is defined exactly once under ``autoinst_amd/csrc`` -- in
``ai_entry.h`` (the host side of one call, the offset-array searches), ``ai_runs.h`` (sorted runs) or ``ai_cells.inc`` (the cell lists)
-- and none of the names its copies had is defined any more."""
import os
import re

import pytest

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "autoinst_amd", "csrc")

# a function definition starts in the first column (calls are indented) and runs to its opening brace without a semicolon
_FUNCTION = r"^(?![/#])\S[^\n;]*\b%s\((?:[^;{]*)%s\) \{"
_STRUCT = r"^struct %s \{"

HELPERS = {
    "ai_entry.h": ["to_device", "upload", "dev_out", "dev_out_if_wanted", "to_caller", "grid_for", "bits_for", "bad_arg", "segment_of",
                   "segment_in"],
    "ai_runs.h": ["scan_flags", "kl_heads", "kv_starts", "kq_compact"],
    "ai_cells.inc": ["sq_dist3", "face_gap", "axis_mag", "knn_insert", "kcell_of", "kq_gather", "pcell_of", "build_cells"],
}
FORMER_NAMES = ["ag_to_device", "gr_to_device", "gr_out", "ag_out_buf", "sp_grid_for", "sp_bits_for", "ag_bad", "gr_bad", "sp_bad",
                "sp_segment_of", "chunk_of", "ag_segment_in", "gr_segment_in", "kf_ggather", "kv_heads", "ks_heads", "ks_starts",
                "ku_compact"]


def _sources():
    out = {}
    for name in sorted(os.listdir(_CSRC)):
        if name.endswith((".hip", ".h", ".inc")):
            with open(os.path.join(_CSRC, name)) as f:
                out[name] = f.read()
    return out


SOURCES = _sources()


def _definitions(pattern):
    return [name for name, text in SOURCES.items() for _ in re.finditer(pattern, text, re.M)]


@pytest.mark.parametrize("header, helper", [(h, n) for h, names in HELPERS.items() for n in names])
def test_a_shared_helper_is_defined_once(header, helper):
    assert _definitions(_FUNCTION % (helper, "")) == [header], helper


def test_sort_pairs_is_defined_once_per_signature():
    assert _definitions(_FUNCTION % ("sort_pairs", r"int bits")) == ["ai_runs.h"]
    assert _definitions(_FUNCTION % ("sort_pairs", r"DevBuf<uint8_t>& tmp")) == ["ai_runs.h"]
    assert len(_definitions(_FUNCTION % ("sort_pairs", ""))) == 2
    # and no point-cloud source spells the two rocPRIM calls of a pair sort out for itself (the affinity and NCut sources have their own)
    ours = ("ai_points.hip", "ai_camera.hip", "ai_scanpool.hip", "ai_finish.hip", "ai_prep.hip", "ai_labels.hip", "ai_merge.hip",
            "ai_aggregate.hip", "ai_ground.hip", "ai_labels_shared.h", "ai_entry.h", "ai_runs.h", "ai_cells.inc")
    assert [f for f in _definitions(r"rocprim::radix_sort_pairs\(") if f in ours] == ["ai_runs.h"] * 2


def test_the_grids_are_defined_once():
    for grid in ("KGrid", "PGrid"):
        assert _definitions(_STRUCT % grid) == ["ai_cells.inc"], grid


@pytest.mark.parametrize("name", FORMER_NAMES)
def test_no_copy_is_left_under_its_former_name(name):
    assert _definitions(_FUNCTION % (name, "")) == [], name
    assert not any(re.search(r"\b%s\b" % name, text) for text in SOURCES.values()), name


def test_the_cell_list_is_a_header():
    # a header under its old file name (tests/points_cases.py reads the grid's limits out of it by that name): no source pastes it
    # inside its own namespace any more
    for name, text in SOURCES.items():
        at = text.find('#include "ai_cells.inc"')
        assert at < 0 or "namespace {" not in text[:at], name
    for header in HELPERS:
        text = SOURCES[header]
        assert "#pragma once" in text and re.search(r"^namespace \{$", text, re.M), header
    assert "#include <rocprim" not in SOURCES["ai_entry.h"] and "#include <rocprim" not in SOURCES["ai_common.h"]
    with open(os.path.join(_CSRC, "Makefile")) as f:
        make = f.read()
    users = {h: sorted(n[:-4] for n, text in SOURCES.items() if n.endswith(".hip") and re.search(r'#include "%s"' % h, text)) for h in HELPERS}
    users["ai_runs.h"] += users["ai_cells.inc"]                      # ai_cells.inc includes the other two,
    users["ai_runs.h"] += ["ai_labels", "ai_merge"]                # ai_labels_shared.h the first two
    users["ai_entry.h"] += users["ai_runs.h"]
    assert all(re.search(r'#include "%s"' % h, SOURCES["ai_cells.inc"]) for h in ("ai_entry.h", "ai_runs.h"))
    assert all(re.search(r'#include "%s"' % h, SOURCES["ai_labels_shared.h"]) for h in ("ai_entry.h", "ai_runs.h"))
    for header, objects in users.items():
        for obj in objects:
            assert any(re.search(r"\b%s\.o\b" % obj, line.split(":")[0]) and header in line.split(":", 1)[1]
                       for line in make.splitlines() if ":" in line and not line.startswith(("#", "\t"))), (header, obj)
