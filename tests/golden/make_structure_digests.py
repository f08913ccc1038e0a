"""Recorder of tests/golden/structure_digests.json: per case of tests/structure_digest_cases.py the digest of the Python generator's
stream (numpy path; the device= path must give the same), the case's k, and -- where a GPU is present -- the digests of the native
generator's arrays without and with the instance column.  Run it on the commit whose behaviour is to be pinned, BEFORE a change to the
generators, never on the code under test:

    python tests/golden/make_structure_digests.py [--out FILE]

Without a GPU the native digests of an existing file are kept as they are."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
DEFAULT = os.path.join(ROOT, "tests", "golden", "structure_digests.json")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=DEFAULT)
    args = ap.parse_args()
    import torch

    from tests import structure_digest_cases as SD

    old = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            old = json.load(f)
    eng = None
    if torch.cuda.is_available():
        import paillier_halo2_amd as pz

        eng = pz.Engine(0)
        eng.bind_torch_stream()
    out = {}
    for cid, kind, kw in SD.CASES:
        sa = SD.stream(kind, kw)
        entry = {"k": SD.pick_k(sa), "stream": SD.stream_digest(sa)}
        assert SD.stream_digest(SD.stream(kind, kw, device="cpu")) == entry["stream"], cid
        for name, expose in (("native", False), ("native_expose", True)):
            if eng is None:
                if name in old.get(cid, {}):
                    entry[name] = old[cid][name]
                continue
            ns = SD.native(eng, kind, kw, entry["k"], expose)
            try:
                entry[name] = SD.native_digest(ns)
            finally:
                ns.free()
        out[cid] = entry
        print(cid, entry, flush=True)
    if eng is not None:
        eng.close()
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
