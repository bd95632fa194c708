"""What the two-stage file decoders (DESIGN sections 16 and 17) share.  A CODEC turns a file into a PACKED FRAME on the host --
a flat uint8 array whose size depends on the geometry only -- and a stacked batch of packed frames of one geometry into uint8
CUDA [N,H,W,3] on the device.  ``jpegdecode`` and ``pngdecode`` each state theirs as a ``Codec``; the batch driver, the checks in
front of the upload and the Pillow fallback are here, once."""
import collections
import io
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

# key: the sample key a packed frame travels under;  host_stage(data) -> packed;  packed_info(packed) -> dict with width and
# height;  batch_geometry(packed_batch) -> tuple starting (width, height), after checking on the host all that the device stage
# relies on;  geometry_header_bytes: the leading bytes of a packed frame that, with its size, identify its geometry;
# device_stage(packed_d, n, geom, out, dev): the launches;  prepare(): called once before the host stage runs in threads
Codec = collections.namedtuple("Codec", "key host_stage packed_info batch_geometry geometry_header_bytes device_stage prepare",
                               defaults=(None,))


def as_bytes(data):
    if isinstance(data, np.ndarray):
        data = np.ascontiguousarray(data, dtype=np.uint8).tobytes()
    return bytes(data)


def pillow_rgb(data):
    from PIL import Image

    return np.array(Image.open(io.BytesIO(data)).convert("RGB"))  # (a writable copy: it becomes a tensor)


def __getattr__(name):
    if name == "CODECS":  # the codecs there are, for looking a sample key up in
        from handobjectconsist_amd.datasets import jpegdecode, pngdecode  # (not at the top: both import this module)

        return jpegdecode.CODEC, pngdecode.CODEC
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def codec_for(data):
    """The codec of a file's bytes: PNG for the full 8-byte signature, JPEG for everything else (whose host stage then says
    what is wrong with it)."""
    from handobjectconsist_amd.datasets import jpegdecode, pngdecode

    return pngdecode.CODEC if bytes(data[:8]) == pngdecode.SIGNATURE else jpegdecode.CODEC


def decode_packed(codec, packed_batch, device):
    """[N, bytes] packed frames of ONE geometry (numpy or CPU tensor) -> uint8 CUDA [N,H,W,3]: the codec's checks on the host,
    one upload, its device stage."""
    if torch.is_tensor(packed_batch):
        if packed_batch.is_cuda:
            raise ValueError("packed_batch lives on the host (its headers are checked there)")
        packed_batch = packed_batch.numpy()
    packed_batch = np.ascontiguousarray(packed_batch)
    if packed_batch.ndim == 2 and packed_batch.shape[0] == 0:
        raise ValueError("an empty packed_batch has no geometry")
    geom = codec.batch_geometry(packed_batch)
    N = packed_batch.shape[0]
    dev = torch.device(device)
    packed_d = torch.from_numpy(packed_batch).to(dev, non_blocking=True)
    out = torch.empty((N, geom[1], geom[0], 3), dtype=torch.uint8, device=dev)
    codec.device_stage(packed_d, N, geom, out, dev)
    return out


def decode_batch(codec, files, device, threads=None, unsupported="raise"):
    """``jpegdecode.decode_batch`` / ``pngdecode.decode_batch`` (whose docstrings say what it does) for any codec: the host
    stage in threads, one ``decode_packed`` call per geometry, Pillow for unsupported files on request."""
    if unsupported not in ("raise", "pillow"):
        raise ValueError("unsupported must be 'raise' or 'pillow'")
    files = [as_bytes(f) for f in files]
    if not files:
        raise ValueError("decode_batch needs at least one file")

    def one(data):
        try:
            return codec.host_stage(data)
        except NotImplementedError:
            if unsupported == "raise":
                raise
            return pillow_rgb(data)  # [H, W, 3]: told apart from a packed frame by its rank

    threads = min(16, len(files)) if threads is None else max(1, int(threads))
    if codec.prepare is not None:
        codec.prepare()
    if threads == 1:
        staged = [one(f) for f in files]
    else:
        with ThreadPoolExecutor(threads) as pool:
            staged = list(pool.map(one, files))
    dev = torch.device(device)
    first, hb = staged[0], codec.geometry_header_bytes
    if all(s.ndim == 1 and s.size == first.size and np.array_equal(s[:hb], first[:hb]) for s in staged):
        return decode_packed(codec, np.stack(staged), dev)  # the usual case: one geometry
    groups, frames = {}, [None] * len(files)
    for i, s in enumerate(staged):
        if s.ndim == 3:
            frames[i] = torch.from_numpy(s).to(dev, non_blocking=True)
        else:
            groups.setdefault((s[:hb].tobytes(), s.size), []).append(i)
    for idxs in groups.values():
        decoded = decode_packed(codec, np.stack([staged[i] for i in idxs]), dev)
        for k, i in enumerate(idxs):
            frames[i] = decoded[k]
    if len({tuple(f.shape) for f in frames}) != 1:
        raise ValueError("decode_batch: the files have different frame sizes")
    return frames[0][None] if len(frames) == 1 else torch.stack(frames)
