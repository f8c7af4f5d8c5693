"""Golden similarity fields, by RUNNING THE REFERENCE (CPU, build container only):
``python tests/golden/make_golden_similarity_field.py`` -> tests/golden/similarity_field_small.npz.

The reference's own ``UFORecon.extract_fields`` (code1/model.py:891-911) with ``UFORecon.query_cond_info`` as its query
function, on ``gather_ref.frame_for(NV)`` for NV = 2, 3, 5 at resolution 9 over the cubes +-1 and +-4: ``u/nv<NV>/b<half>``.

ONE stub.  As written the method does not run: with ``extract_similarity=True`` ``camera.get_coord_ref_ndc`` returns ONE
tensor and ``query_cond_info`` unpacks three (``ValueError: not enough values to unpack (expected 3, got 1)``; the call site
at model.py:618-626 is commented out).  For the run, ``code1.model.camera.get_coord_ref_ndc`` is wrapped so that in that mode
its result ``r`` comes back as ``(r, None, None)``; nothing else of the reference is touched.
"""
from __future__ import annotations

import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
warnings.filterwarnings("ignore")

from ref_harness import build_reference_model  # noqa: E402
import gather_ref  # noqa: E402

OUT = os.path.join(HERE, "similarity_field_small.npz")
NVS = (2, 3, 5)
HALVES = (1, 4)
RESOLUTION = 9


def stub_unpack():
    import code1.model as ref_model

    inner = ref_model.camera.get_coord_ref_ndc

    def get_coord_ref_ndc(*a, **k):
        r = inner(*a, **k)
        return (r, None, None) if k.get("extract_similarity", False) else r

    ref_model.camera.get_coord_ref_ndc = get_coord_ref_ndc


def main():
    g = {}
    stubbed = False
    for NV in NVS:
        model = build_reference_model(0, test_n_view=NV)
        if not stubbed:
            stub_unpack()
            stubbed = True
        fr = gather_ref.frame_for(NV)
        for half in HALVES:
            lo = torch.tensor([-float(half)] * 3, dtype=torch.float32)
            hi = torch.tensor([float(half)] * 3, dtype=torch.float32)
            u = model.extract_fields(lo, hi, RESOLUTION, model.query_cond_info, "cpu", fr.batch, fr.match_feature)
            assert u.shape == (RESOLUTION,) * 3 and u.dtype == np.float32
            g[f"u/nv{NV}/b{half}"] = u
    np.savez_compressed(OUT, **g)
    print(OUT, os.path.getsize(OUT), "bytes,", len(g), "arrays")


if __name__ == "__main__":
    main()
