"""Generate tests/golden/workspace_sizes.json: what every sizing entry point of libmeshraster_hip.so answers on a grid of
shapes -- sizes, offsets inside a workspace where an entry point hands them out, and the error codes of negative and zero
arguments.  None of these entry points touches a device.

    PYTHONDONTWRITEBYTECODE=1 HOC_LIB_PATH=<library to record> python tests/golden/make_golden_workspace_sizes.py [output path [source hash]]

(source hash: ``build.source_hash()`` of the tree the library was built from, when that is not the tree at hand.)

The file is a record of the library as it was BEFORE the entry points' host side moved onto csrc/host_layout.hpp (its
``build.source_hash()`` is stored with it), when most workspaces had their size and their partition written out twice by
hand.  It is not regenerated from later code: a value that differs is a workspace whose size, padding or region order
changed.  tests/test_workspace_sizes_host.py imports the grid and the runner from this file.

The grid holds the shapes where padding matters: batches whose arrays end off the 256-byte grid (1, 3, 33) and on it (64,
192), face counts around 256 and the meshes of the training path (1538, 3076, 7104), rasters of a pixel or two (strip
weights outnumber pixel quads), rasters that are no multiple of the 32 x 8 tile (30, 36, 100, 257) and the benchmark's
(256, 480, 640), frames from 1 x 1 to 256 x 256.  The three-argument render entry points take the grid pair by pair
(every batch x faces, batch x raster and faces x raster combination at two or three values of the third argument).
"""
import ctypes
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
PATH = os.path.join(HERE, "workspace_sizes.json")

BATCHES = (0, 1, 2, 3, 8, 33, 64, 192)
FACES = (0, 1, 5, 255, 256, 257, 1538, 3076, 7104)
RASTERS = (1, 2, 3, 6, 30, 36, 100, 256, 257, 480, 640)
FRAMES = ((1, 1), (3, 5), (17, 9), (256, 256))  # (height, width)


def _bad(base):
    """`base` with each argument in turn set to -1 and to 0"""
    out = []
    for k in range(len(base)):
        for v in (-1, 0):
            out.append(base[:k] + (v,) + base[k + 1:])
    return out


def _render_grid():
    rows = set()
    rows.update((b, f, r) for b in BATCHES for f in FACES for r in (2, 36, 256))
    rows.update((b, f, r) for b in BATCHES for f in (5, 3076) for r in RASTERS)
    rows.update((b, f, r) for b in (1, 33) for f in FACES for r in RASTERS)
    return sorted(rows) + [(2, 10, 36)] + _bad((2, 10, 36)) + [(2, 10, 16384), (2, 10, 16385)]


def _stem_grid():
    shapes = [(b, c, h, w) for b in BATCHES for c in (3, 64) for (h, w) in FRAMES + ((112, 112), (113, 111))]
    return shapes + _bad((2, 64, 112, 112))


# entry point -> argument tuples (all int); the value recorded is the int64 the entry point returns
PLAIN = {
    "mr_render_workspace_bytes": _render_grid(),
    "mr_render_clear_bytes": _render_grid(),
    "mr_render_backward_workspace_bytes": _render_grid(),
    "mr_render_backward_list_workspace_bytes": [(b, f) for b in BATCHES for f in FACES] + _bad((3, 5)),
    "mr_pair_consist_workspace_bytes": [(b, h, w) for b in BATCHES for (h, w) in FRAMES + tuple((r, r) for r in RASTERS)] + _bad((2, 17, 9)),
    "mr_pair_consist_tiles_workspace_bytes": [(b, r) for b in BATCHES for r in RASTERS] + _bad((2, 36)),
    "mr_flow_pair_scatter_work_bytes": [(b, r) for b in BATCHES for r in RASTERS] + _bad((2, 36)),
    "mr_mano_workspace_floats": [(b,) for b in BATCHES + (-1, 31, 32, 65)],
    "mr_mano_full_workspace_floats": [(b,) for b in BATCHES + (-1, 31, 32, 65)],
    "mr_frames_to_batch_workspace_bytes": [(n, h, w) for n in BATCHES for (h, w) in FRAMES] + _bad((2, 17, 9)),
    "mr_frames_color_augment_workspace_bytes": [(n, h, w) for n in BATCHES for (h, w) in FRAMES] + _bad((2, 17, 9)),
    "mr_jpeg_packed_bytes": [(w, h, c, lh, lv) for (h, w) in FRAMES for c in (1, 3) for (lh, lv) in ((1, 1), (2, 1), (2, 2), (1, 2), (4, 1))]
                            + _bad((9, 17, 3, 2, 2)),
    "mr_jpeg_reconstruct_workspace_bytes": [(n, w, h, c, lh, lv) for n in (0, 1, 3, 33) for (h, w) in FRAMES for c in (1, 3)
                                            for (lh, lv) in ((1, 1), (2, 1), (2, 2))] + _bad((2, 9, 17, 3, 2, 2)),
    "mr_png_packed_bytes": [(w, h, c) for (h, w) in FRAMES + ((10752, 10752), (10753, 1)) for c in (1, 2, 3, 4)] + _bad((9, 17, 3)),
    "mr_png_unfilter_workspace_bytes": [(n, w, h, c) for n in (0, 1, 3, 33) for (h, w) in FRAMES for c in (1, 3, 4)] + _bad((2, 9, 17, 3)),
    "mr_bn_act_backward_workspace_bytes": [(b, c) for b in BATCHES for c in (1, 3, 64, 256, 1024, 2048)] + _bad((2, 64)),
    "mr_bn_add_bn_act_backward_workspace_bytes": [(b, c) for b in BATCHES for c in (1, 3, 64, 256, 1024, 2048)] + _bad((2, 64)),
    "mr_stem_pool_records_bytes": _stem_grid(),
    "mr_stem_pool_backward_workspace_bytes": _stem_grid(),
    "mr_stem_conv_wrw_workspace_bytes": [(b, c, h, w) for b in BATCHES for c in (3, 64) for (h, w) in FRAMES + ((224, 224), (225, 223))]
                                        + _bad((2, 64, 224, 224)),
}

# mr_pair_step_sizes: (batch_size, num_verts_a, num_verts_b, num_hand_faces, num_obj_faces, fill_back, image_size, height, width,
# jitter_channels, criterion, reserved)
_MESHES = ((778, 1000, 1538, 2000, 1), (778, 8, 1538, 12, 0), (0, 3, 0, 1, 1))
PAIR_STEP = ([(b, va, vb, fh, fo, fill, r, r, r, 3, 0, 0) for b in BATCHES for (va, vb, fh, fo, fill) in _MESHES for r in RASTERS]
             + [(2, 778, 1000, 1538, 2000, 1, 256, 200, 180, 1, crit, res) for crit in (0, 1, 2, -1) for res in (0, 1, 0x201, 0x200, 0x10000, 3)]
             + [(2, 778, 1000, 1538, 2000, 1, 256, h, w, jc, 0, 0) for (h, w, jc) in ((256, 1, 3), (257, 256, 3), (0, 256, 3), (256, 256, 2), (4, 2, 1))]
             + [(2, 778, 2000, 1538, 2000, 1, 256, 256, 256, 3, 0, 0), (1 << 20, 1, 1, 1, 1, 0, 4, 4, 4, 1, 0, 0), ((1 << 20) + 1, 1, 1, 1, 1, 0, 4, 4, 4, 1, 0, 0)]
             + _bad((2, 778, 1000, 1538, 2000, 1, 36, 36, 36, 3, 0, 0)))
_PS_FIELDS = ("batch_size", "num_verts_a", "num_verts_b", "num_hand_faces", "num_obj_faces", "fill_back", "image_size", "height",
              "width", "jitter_channels", "criterion", "reserved")


def run(lib):
    """{entry point: [[arguments..., results...], ...]} from a loaded library (handobjectconsist_amd._lib.load())."""
    from handobjectconsist_amd.warping.pairstep import MrPairStep

    out = {}
    for name, grid in PLAIN.items():
        fn = getattr(lib, name)
        out[name] = [list(args) + [int(fn(*args))] for args in grid]
    # mr_render_tile_list on a fake base of 256, as pair_step_layout and _lib.has_tile_list call it: return code, the two
    # addresses it hands out and the capacity (zeros where it refuses)
    rows = []
    for args in _render_grid():
        hdr, ents, cap = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int64()
        rc = lib.mr_render_tile_list(ctypes.c_void_p(256), *args, ctypes.byref(hdr), ctypes.byref(ents), ctypes.byref(cap))
        rows.append(list(args) + [int(rc), int(hdr.value or 0), int(ents.value or 0), int(cap.value)])
    out["mr_render_tile_list"] = rows
    rows = []
    for args in PAIR_STEP:
        st = MrPairStep()
        for n, v in zip(_PS_FIELDS, args):
            setattr(st, n, int(v))
        sc, sv, th = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        rc = lib.mr_pair_step_sizes(ctypes.byref(st), ctypes.byref(sc), ctypes.byref(sv), ctypes.byref(th))
        rows.append(list(args) + [int(rc), int(sc.value), int(sv.value), int(th.value)])
    out["mr_pair_step_sizes"] = rows
    th, tw, wg = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    rc = lib.mr_stem_conv_wrw_tiling(ctypes.byref(th), ctypes.byref(tw), ctypes.byref(wg))
    out["mr_stem_conv_wrw_tiling"] = [[int(rc), th.value, tw.value, wg.value]]
    return out


def main():
    from handobjectconsist_amd import _lib, build

    record = {"library": os.path.basename(_lib.LIB_PATH), "source_hash": sys.argv[2] if len(sys.argv) > 2 else build.source_hash(),
              "entries": run(_lib.load())}
    path = sys.argv[1] if len(sys.argv) > 1 else PATH
    with open(path, "w") as fh:
        fh.write("{\n")
        fh.write(' "library": %s,\n "source_hash": %s,\n "entries": {\n' % (json.dumps(record["library"]), json.dumps(record["source_hash"])))
        names = list(record["entries"])
        for name in names:
            rows = ",\n".join("   " + json.dumps(r, separators=(",", ":")) for r in record["entries"][name])
            fh.write('  %s: [\n%s\n  ]%s\n' % (json.dumps(name), rows, "," if name != names[-1] else ""))
        fh.write(" }\n}\n")
    print(path, sum(len(v) for v in record["entries"].values()), "rows")


if __name__ == "__main__":
    main()
