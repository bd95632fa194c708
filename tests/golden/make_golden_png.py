"""Generator of tests/golden/png_pil.npz: the shared PNG cases of tests/png_ref.py as recorded data -- every case's stream
(uint8; hand-made with forced row filters, or as the installed Pillow encodes it) and the pixels the installed Pillow decodes
from it (``Image.open(...).convert("RGB")``), plus one palette stream for the mixed ``decode_batch`` test.  Pillow only --
no kernel, no numpy restatement of the unfilter; the GPU tests then do not depend on the GPU box's Pillow build.

    python tests/golden/make_golden_png.py
"""
import io
import json
import os
import sys

import numpy as np
import PIL
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import png_ref as R  # noqa: E402  (the case list, the content generators and the stream writer only)

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "png_pil.npz")


def main():
    arrays, names = {}, []
    streams = R.all_streams()
    streams["palette"] = R.palette_stream()
    for name, data in streams.items():
        if name != "palette":
            names.append(name)
        arrays[name + "_stream"] = np.frombuffer(data, np.uint8)
        arrays[name + "_rgb"] = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
    arrays["meta"] = np.array(json.dumps(dict(names=names, pillow=PIL.__version__)))
    np.savez_compressed(OUT, **arrays)
    print(OUT, os.path.getsize(OUT), "bytes,", len(names), "cases")


if __name__ == "__main__":
    main()
