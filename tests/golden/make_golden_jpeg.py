"""Generator of tests/golden/jpeg_pil.npz: the shared JPEG cases of tests/jpeg_ref.py as recorded data -- every case's stream
as the installed Pillow encodes it (uint8) and the pixels the installed Pillow decodes from it
(``Image.open(...).convert("RGB")``), plus one progressive stream for the mixed ``decode_batch`` test.  Pillow only -- no
kernel, no numpy restatement; the GPU tests then do not depend on the GPU box's Pillow build.

    python tests/golden/make_golden_jpeg.py
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
from tests import jpeg_ref as R  # noqa: E402  (the case list and the content generator only)

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "jpeg_pil.npz")


def main():
    arrays, names = {}, []
    for case in R.case_list():
        data = R.encode(case)
        names.append(case[0])
        arrays[case[0] + "_stream"] = np.frombuffer(data, np.uint8)
        arrays[case[0] + "_rgb"] = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
    buf = io.BytesIO()
    Image.fromarray(R.content(48, 40, 31)).save(buf, "JPEG", quality=75, subsampling=2, progressive=True)
    arrays["progressive_stream"] = np.frombuffer(buf.getvalue(), np.uint8)
    arrays["progressive_rgb"] = np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB"))
    arrays["meta"] = np.array(json.dumps(dict(names=names, pillow=PIL.__version__)))
    np.savez_compressed(OUT, **arrays)
    print(OUT, os.path.getsize(OUT), "bytes,", len(names), "cases")


if __name__ == "__main__":
    main()
