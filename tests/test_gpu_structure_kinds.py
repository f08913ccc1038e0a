"""GPU: the native structure generator (csrc/pz_structure.hip) against the Python one on EVERY circuit kind, at the small shapes of
tests/structure_digest_cases.py, without and with the instance column -- array for array, as tests/test_gpu_structure.py does for the
encrypt and add circuits -- and against the digests of its own arrays recorded before the generators were split into shared parts
(tests/golden/structure_digests.json), so that a mistake made the same way in both generators cannot pass."""
import json
import os

import numpy as np
import pytest

from tests import structure_digest_cases as SD

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "structure_digests.json")) as _f:
    GOLDEN = json.load(_f)


@pytest.fixture(scope="module")
def eng():
    import paillier_halo2_amd as pz

    e = pz.Engine(0)
    e.bind_torch_stream()
    yield e
    e.close()


@pytest.fixture(scope="module")
def streams():
    """the Python generator's stream per case, made once and left unchanged"""
    made = {}

    def get(cid, kind, kw):
        if cid not in made:
            made[cid] = SD.stream(kind, kw)
        return made[cid]

    return get


@pytest.mark.parametrize("expose", [False, True], ids=["plain", "expose"])
@pytest.mark.parametrize("cid,kind,kw", SD.CASES, ids=SD.IDS)
def test_native_structure_equals_the_python_generator_and_what_it_was(eng, streams, cid, kind, kw, expose):
    from paillier_halo2_amd import circuit_structure as CS

    sa = streams(cid, kind, kw)
    k = SD.pick_k(sa)
    assert k == GOLDEN[cid]["k"]
    cs, starts = CS.columns(sa, k, SD.LB, device="cpu", expose=expose)
    assert cs.n_adv <= SD.MAX_ADVICE
    ns = SD.native(eng, kind, kw, k, expose)
    try:
        assert (ns.n_cells, ns.n_lookups, ns.n_steps_g, ns.n_steps_r) == (sa.n_cells, sa.lookup_src.shape[0], sa.n_steps_g, sa.n_steps_r)
        assert (ns.n_adv, ns.n_adv_used, ns.n_lk, ns.max_rows, ns.m) == (cs.n_adv, cs.n_adv_used, cs.n_lk, cs.max_rows, cs.m)
        assert ns.constants() == [int(c) for c in cs.constants]          # same constants in the same rows of the constants column
        assert ns.starts().tolist() == starts.tolist()
        sel, mc, mr = ns.download()
        assert np.array_equal(sel, cs.selectors)
        assert np.array_equal(mc, cs.map_col.view(np.uint32)) and np.array_equal(mr, cs.map_row.view(np.uint32))
        if expose:
            assert ns.public_cells() == cs.public_cells
        assert SD.native_digest(ns) == GOLDEN[cid]["native_expose" if expose else "native"]
    finally:
        ns.free()
