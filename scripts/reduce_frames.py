"""Make the reduced copy of a tree of frames, the counterpart of the reference's reduce_fphab.py
(``Image.open(src).resize((480, 270), Image.BILINEAR).save(dst)`` per file): decode and resize run on the GPU, byte for byte
what Pillow gives (DESIGN sections 16, 17, 21); Pillow encodes the result under the source's name with its default parameters,
as the reference does.

    python scripts/reduce_frames.py SRC DST --size 480 270 [--batch 32] [--device cuda:0]

mirrors SRC's tree of .jpg / .jpeg / .png files under DST and skips files that exist there.  Files are grouped by format and
geometry; a group goes through ``framecodec.decode_batch(..., unsupported="pillow")`` (the host stage in threads, one upload,
one reconstruct / unfilter launch) and one ``frames.resize`` launch.

``reduce_tree`` is the walk and the batching; it takes the decode + resize of one group as a callable, so that a machine
without a GPU can drive it (tests/test_resize_host.py injects Pillow)."""
import argparse
import io
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

EXTENSIONS = (".jpg", ".jpeg", ".png")


def frame_files(src):
    """relative paths of the frame files under ``src``, sorted (directories and names in lexical order)"""
    out = []
    for dirpath, dirnames, filenames in os.walk(src):
        dirnames.sort()
        for name in sorted(filenames):
            if name.lower().endswith(EXTENSIONS):
                out.append(os.path.relpath(os.path.join(dirpath, name), src))
    return out


def device_reduce(device="cuda:0", threads=None):
    """(files' bytes of one format and geometry, (W, H)) -> uint8 [N, H, W, 3] through the device path"""
    from handobjectconsist_amd.datasets import framecodec, frames

    def reduce(files, size):
        decoded = framecodec.decode_batch(framecodec.codec_for(files[0]), files, device, threads, unsupported="pillow")
        return frames.resize(decoded, size).cpu().numpy()

    return reduce


def reduce_tree(src, dst, size, reduce, batch=32, log=None):
    """Mirror ``src``'s frame files under ``dst`` at ``size`` = (W, H).  ``reduce(files, size)``: the bytes of up to ``batch``
    files of ONE format and geometry -> their resized frames, uint8 [N, H, W, 3].  Files that exist under ``dst`` are
    skipped (a file is written under a temporary name and renamed: an interrupted run leaves no half-written frame that a
    later run would skip).  Returns {"written", "skipped", "groups": calls of ``reduce``}."""
    from PIL import Image

    size = (int(size[0]), int(size[1]))
    if batch < 1:
        raise ValueError("batch must be at least 1")
    stats = {"written": 0, "skipped": 0, "groups": 0}
    pending = {}  # (is PNG, width, height) -> [(relative path, bytes)]

    def flush(key):
        items = pending.pop(key)
        out = np.asarray(reduce([data for _, data in items], size))
        if out.shape != (len(items), size[1], size[0], 3) or out.dtype != np.uint8:
            raise ValueError(f"reduce returned {out.dtype} {list(out.shape)} for {len(items)} files at {size[0]} x {size[1]}")
        stats["groups"] += 1
        for (rel, _), frame in zip(items, out):
            target = os.path.join(dst, rel)
            os.makedirs(os.path.dirname(target) or ".", exist_ok=True)
            head, name = os.path.split(target)
            tmp = os.path.join(head, ".part-" + name)  # (the extension stays: Pillow takes the format from it)
            Image.fromarray(frame).save(tmp)
            os.replace(tmp, target)
            stats["written"] += 1
        if log:
            log(f"{stats['written']} written, {stats['skipped']} skipped")

    for rel in frame_files(src):
        if os.path.exists(os.path.join(dst, rel)):
            stats["skipped"] += 1
            continue
        with open(os.path.join(src, rel), "rb") as fh:
            data = fh.read()
        with Image.open(io.BytesIO(data)) as im:  # (the headers only)
            key = (im.format == "PNG",) + tuple(im.size)
        pending.setdefault(key, []).append((rel, data))
        if len(pending[key]) == batch:
            flush(key)
    for key in sorted(pending):
        flush(key)
    return stats


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("src")
    ap.add_argument("dst")
    ap.add_argument("--size", type=int, nargs=2, default=(480, 270), metavar=("W", "H"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--threads", type=int, default=None)
    a = ap.parse_args()
    print(reduce_tree(a.src, a.dst, a.size, device_reduce(a.device, a.threads), a.batch, log=print))


if __name__ == "__main__":
    main()
