"""Generator of tests/golden/resize_pil.npz: the shared resize cases of tests/resize_ref.py as recorded data -- per case the
geometry, the seed, the content kind and what the installed Pillow's ``Image.resize(size, Image.BILINEAR)`` makes of that
content (uint8 [H,W,3]).  1920 x 1080 -> 480 x 270 is recorded as the SHA-256 of Pillow's bytes only, and so is the random
content of 640 x 480 -> 480 x 270 (390 KB that do not compress).  Pillow only -- no kernel, no numpy restatement of the
resampling; the GPU tests then do not depend on the GPU box's Pillow build.

    python tests/golden/make_golden_resize.py
"""
import json
import os
import sys

import numpy as np
import PIL
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import resize_ref as R  # noqa: E402  (the case list and the contents generator only)

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "resize_pil.npz")


def main():
    arrays, meta = {}, []
    for geom, kind, seed in R.cases():
        src = R.contents(kind, seed, geom[0], geom[1])[0]
        out = np.asarray(Image.fromarray(src).resize((geom[2], geom[3]), Image.BILINEAR))
        assert out.shape == (geom[3], geom[2], 3) and out.dtype == np.uint8
        key = R.case_key(geom, kind, seed)
        entry = dict(geometry=list(geom), kind=kind, seed=seed, key=key)
        if R.hash_only(geom, kind):
            entry["sha256"] = R.sha256(out)
        else:
            arrays[key] = out
        meta.append(entry)
    arrays["meta"] = np.array(json.dumps(dict(cases=meta, pillow=PIL.__version__)))
    np.savez_compressed(OUT, **arrays)
    print(OUT, os.path.getsize(OUT), "bytes,", len(meta), "cases")


if __name__ == "__main__":
    main()
