"""The Python structure generator (paillier_halo2_amd/circuit_structure.py::stream_structure) pinned, on every circuit kind, to what it
gave before its one long function was split into shared parts: SHA-256 over src, gate_mask, lookup_src, the constants, result_cell, the
step counts and public_cells must equal tests/golden/structure_digests.json -- recorded by tests/golden/make_structure_digests.py on the
commit before the split --, on the numpy path and on the device= (torch) tiling path."""
import json
import os

import pytest

from tests import structure_digest_cases as SD

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "structure_digests.json")) as _f:
    GOLDEN = json.load(_f)


def test_the_golden_file_covers_the_case_list():
    assert sorted(GOLDEN) == sorted(SD.IDS)


@pytest.mark.parametrize("device", [None, "cpu"], ids=["numpy", "torch"])
@pytest.mark.parametrize("cid,kind,kw", SD.CASES, ids=SD.IDS)
def test_stream_structure_is_what_it_was(cid, kind, kw, device):
    assert SD.stream_digest(SD.stream(kind, kw, device=device)) == GOLDEN[cid]["stream"]
