"""Records tests/golden/nbest_routes.npz, the fixture of tests/test_hip_nbest_routes.py: every call of that file's grid (taken from
there, with its models, LM and graphs) on cuda:0, as bit patterns.  Run it at the commit whose behaviour is to be pinned, TWICE in two
processes: the fixture is valid only where both recordings hold the same bits.
usage: python tools/record_nbest_routes.py OUT.npz [--against OTHER.npz]
  --against: also compares with an earlier recording, lists every field that differs and exits with 1 if any does"""
import argparse
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
import test_hip_nbest_routes as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("out")
ap.add_argument("--against")
args = ap.parse_args()

results = {(name, call): R.fields(R.decode(name, route, spec)) for name in R.MODELS for call, route, spec in R.GRID}
torch.cuda.synchronize()
arrays = R.pack(results)
Path(args.out).parent.mkdir(parents=True, exist_ok=True)
np.savez_compressed(args.out, **arrays)
print(f"{len(results)} calls, {sum(len(f) for f in results.values())} fields, {Path(args.out).stat().st_size} bytes in {args.out}")
if args.against:
    with np.load(args.against) as z:
        other = {k: z[k] for k in z.files}
    bad = sorted(k for k in set(arrays) | set(other) if k not in arrays or k not in other or not np.array_equal(arrays[k], other[k]))
    for k in bad:
        if k in arrays and k in other and k != "layout":
            at = 0
            for field, _, shape in R.json.loads(str(arrays["layout"]))[k]:
                size = int(np.prod(shape))
                if arrays[k].shape != other[k].shape or not np.array_equal(arrays[k][at:at + size], other[k][at:at + size]):
                    print(f"differs: {k} {field}")
                at += size
        else:
            print(f"differs: {k}")
    print(f"{len(bad)} of {len(arrays)} arrays differ from {args.against}")
    sys.exit(1 if bad else 0)
