"""A synthetic ``pose_dataset`` with the accessor protocol of the reference's dataset classes
(meshreg/datasets/ho3dv2.py: get_image :299, get_joints3d :314, get_dist_idx :283, ...): frame pairs of
the synthetic hand + object scene as 'consecutive video frames' of a camera with a larger sensor than the
network input, so that the crop / augmentation path has real work to do.  Stands in for FPHAB / HO3D,
which cannot be shipped."""
import io

import numpy as np

from handobjectconsist_amd.datasets import framecodec
from handobjectconsist_amd.utils import synth


def procedural_models(count, seed=0):
    """``count`` closed meshes of different sizes: ellipsoids of a few centimetres, model j a (4 + 3 j) x (6 + 5 j) latitude /
    longitude grid -- 20, 68, 146, ... vertices, twice as many faces less four -- outward-facing, float32 / int32."""
    rng = np.random.default_rng([seed, 35])
    models = []
    for j in range(int(count)):
        lat, lon = 4 + 3 * j, 6 + 5 * j
        radii = rng.uniform(0.03, 0.06, 3)
        th = np.pi * np.arange(1, lat) / lat
        ph = 2 * np.pi * np.arange(lon) / lon
        ring = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.sin(th), np.sin(ph)), np.outer(np.cos(th), np.ones(lon))], -1)
        verts = np.concatenate([[[0, 0, 1.0]], ring.reshape(-1, 3), [[0, 0, -1.0]]]) * radii
        at = lambda i, k: 1 + i * lon + k % lon
        south = 1 + (lat - 1) * lon
        faces = [[0, at(0, k), at(0, k + 1)] for k in range(lon)]
        for i in range(lat - 2):
            for k in range(lon):
                faces += [[at(i, k), at(i + 1, k), at(i + 1, k + 1)], [at(i, k), at(i + 1, k + 1), at(i, k + 1)]]
        faces += [[south, at(lat - 2, k + 1), at(lat - 2, k)] for k in range(lon)]
        models.append((verts.astype(np.float32), np.array(faces, np.int32)))
    return models


class SynthPoseDataset:
    has_dist2strong = False

    def __init__(self, num_pairs=4, frame_size=(640, 480), seed=0, sides=("right",), jpeg_quality=None, jpeg_subsampling=2,
                 png_compress_level=None, mano_layer=None, file_scale=1, obj_models=None):
        """2 * num_pairs frames: frame 2k and 2k + 1 are the two time steps of scene k.
        jpeg_quality (None: frames are arrays, as ever): the frames exist as JPEG files' bytes, encoded by Pillow at this
        quality and ``jpeg_subsampling`` (0 / 1 / 2: 4:4:4 / 4:2:2 / 4:2:0) -- ``get_image_bytes(idx)`` returns them (the
        accessor ``HandObjSet(decode="device")`` needs) and ``get_image(idx)`` Pillow's decode of those same bytes.
        png_compress_level (None, or 0..9; not together with jpeg_quality): the same for PNG files, written by Pillow at this
        zlib level -- lossless, so ``get_image(idx)`` equals the array.
        mano_layer (None: the hand vertices are the scene's, as ever): a CPU ``SynthManoLayer`` as the reference's datasets
        build it (``use_pca=False, flat_hand_mean=True, center_idx=None``, fhbhands.py:103-108).  Every frame then has a MANO
        annotation (fullpose [48], trans [3], shape [10]) drawn from a generator seeded with ``seed``: ``get_hand_info(idx)``
        returns it (the reference's accessor, fhbhands.py:367-370) and ``get_hand_verts3d(idx)`` evaluates the layer on it
        (``manogt.hand_verts_host``, fhbhands.py:355-359).  Everything else is untouched.
        file_scale (1: as ever; an integer k above 1): the frames -- arrays, JPEG or PNG files -- are k times ``frame_size``
        a side, while the intrinsics, the boxes and every other annotation stay in ``frame_size`` coordinates: FPHAB as
        downloaded (1920 x 1080 files, annotations the reference scales by ``reduce_factor = 1 / 4``, fhbhands.py:110-130),
        for ``HandObjSet(frame_size=...)``.
        obj_models (None: the object is the scene's, as ever): a list of (verts [V,3], faces [F,3]) models, or a count k of
        procedural ones of different sizes (``procedural_models``).  They form ``self.obj_bank`` (``objgt.ObjectBank``); every
        scene then has a model id and each of its two frames a rigid placement [A | b] near the scene's object (float64), drawn
        from a generator seeded with ``seed``: ``get_obj_info(idx)`` returns them (the accessor ``HandObjSet(obj_geometry="device")`` needs), and
        ``get_obj_verts_trans`` / ``get_obj_faces`` / ``get_obj_verts_can`` evaluate the same annotation through the bank's host
        functions.  Everything else is untouched."""
        if jpeg_quality is not None and png_compress_level is not None:
            raise ValueError("jpeg_quality and png_compress_level: the frames are files of one format")
        if int(file_scale) != file_scale or file_scale < 1:
            raise ValueError(f"file_scale must be an integer of at least 1, got {file_scale!r}")
        self.file_scale = int(file_scale)
        self.frame_size = tuple(frame_size)  # (W, H)
        W, H = self.frame_size
        scene = synth.random_scene(num_pairs, seed=seed, image_size=256)
        rng = np.random.default_rng(seed)
        self.hand, self.obj, self.K = [], [], []
        for k in range(num_pairs):
            for f in ("1", "2"):
                self.hand.append(scene["hand_verts" + f][k])
                self.obj.append(scene["obj_verts" + f][k])
                K = scene["K" + f][k].copy()
                K[0, 2] += (W - 256) / 2  # principal point of the larger sensor
                K[1, 2] += (H - 256) / 2
                self.K.append(K)
        self.obj_faces = scene["obj_faces"]
        self.frames = rng.integers(0, 256, (2 * num_pairs, H * self.file_scale, W * self.file_scale, 3), dtype=np.uint8)
        self.sides = [sides[i % len(sides)] for i in range(2 * num_pairs)]
        self.files = None  # the frames as files' bytes, where a format is chosen
        save = None
        if jpeg_quality is not None:
            save = dict(format="JPEG", quality=int(jpeg_quality), subsampling=int(jpeg_subsampling))
        if png_compress_level is not None:
            save = dict(format="PNG", compress_level=int(png_compress_level))
        if save is not None:
            from PIL import Image

            self.files = []
            for frame in self.frames:
                buf = io.BytesIO()
                Image.fromarray(frame).save(buf, **save)
                self.files.append(buf.getvalue())
        obj_all = np.concatenate(self.obj)
        self.can_trans = obj_all.mean(0)
        self.can_scale = float(np.linalg.norm(obj_all - self.can_trans, axis=1).max())
        self.mano_layer, self.mano_infos = mano_layer, None
        if mano_layer is not None:
            if mano_layer.use_pca:
                raise ValueError("mano_layer must take the full axis-angle pose (use_pca=False), as the datasets' layer does")
            mrng = np.random.default_rng([seed, 48])  # (a generator of its own: the frames above do not move)
            self.mano_infos = []
            for k in range(2 * num_pairs):
                fullpose = np.concatenate([mrng.standard_normal(3) * 0.5, mrng.standard_normal(45) * 0.2])
                # the annotated translation: where the scene's hand is (in front of the camera, metres)
                trans = self.hand[k].mean(0) + mrng.standard_normal(3) * 0.01
                self.mano_infos.append({"fullpose": fullpose.astype(np.float32), "trans": trans.astype(np.float32),
                                        "shape": (mrng.standard_normal(10) * 0.5).astype(np.float32)})

        self.obj_bank, self.obj_infos = None, None
        if obj_models is not None:
            from handobjectconsist_amd.datasets import objgt

            models = procedural_models(obj_models, seed) if isinstance(obj_models, (int, np.integer)) else obj_models
            self.obj_bank = objgt.ObjectBank(models)
            orng = np.random.default_rng([seed, 34])  # (a generator of its own: the frames above do not move)
            self.obj_infos = []
            for k in range(2 * num_pairs):
                if k % 2 == 0:  # the two time steps of a scene show one model, turned a little further
                    model, turn = int(orng.integers(len(self.obj_bank))), orng.standard_normal(3) * 0.7
                w = turn + orng.standard_normal(3) * 0.05  # axis-angle -> rotation (Rodrigues, float64)
                t = np.linalg.norm(w)
                K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / t
                R = np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K.dot(K)
                # the placement: where the scene's object is (in front of the camera, metres)
                b = self.obj[k].mean(0) + orng.standard_normal(3) * 0.01
                self.obj_infos.append((model, np.concatenate([R, b[:, None]], 1)))

    def __len__(self):
        return len(self.frames)

    def get_image(self, idx):
        if self.files is not None:
            return framecodec.pillow_rgb(self.files[idx])
        return self.frames[idx]

    def get_image_bytes(self, idx):
        if self.files is None:
            raise RuntimeError("SynthPoseDataset(jpeg_quality=None, png_compress_level=None) holds arrays, not files")
        return self.files[idx]

    def get_sides(self, idx):
        return self.sides[idx]

    def get_camintr(self, idx):
        return self.K[idx]

    def _proj(self, idx, pts):
        h = self.K[idx].dot(pts.T).T
        return h[:, :2] / h[:, 2:]

    def get_center_scale(self, idx):
        """Square box around the projected hand + object, 1.5x loose (what the datasets' own boxes are)."""
        p = self._proj(idx, np.concatenate([self.hand[idx], self.obj[idx]]))
        lo, hi = p.min(0), p.max(0)
        return ((lo + hi) / 2).astype(np.float32), float(1.5 * (hi - lo).max())

    def get_joints3d(self, idx):
        return self.hand[idx][:21].copy()

    def get_hand_verts3d(self, idx):
        if self.mano_layer is not None:
            from handobjectconsist_amd.datasets import manogt

            pose, trans, shape = self.get_hand_info(idx)
            return manogt.hand_verts_host(self.mano_layer, pose[None], shape[None], trans[None])[0]
        return self.hand[idx].copy()

    def get_hand_info(self, idx):
        if self.mano_infos is None:
            raise RuntimeError("SynthPoseDataset(mano_layer=None) holds no MANO annotations")
        info = self.mano_infos[idx]
        return info["fullpose"], info["trans"], info["shape"]

    def get_obj_info(self, idx):
        if self.obj_infos is None:
            raise RuntimeError("SynthPoseDataset(obj_models=None) holds no model ids")
        return self.obj_infos[idx]

    def get_obj_verts_trans(self, idx):
        if self.obj_bank is not None:
            return self.obj_bank.verts_trans(*self.obj_infos[idx])
        return self.obj[idx].copy()

    def get_obj_faces(self, idx):
        if self.obj_bank is not None:
            return self.obj_bank.faces[self.obj_infos[idx][0]]
        return self.obj_faces

    def get_obj_verts_can(self, idx):
        if self.obj_bank is not None:
            return self.obj_bank.canonical(self.obj_infos[idx][0])
        return (self.obj[idx] - self.can_trans) / self.can_scale, self.can_trans, self.can_scale

    # the 2-D annotations, in ho3dv2.py's form (:309-312, 350-354, 454-458): ``project`` on the accessor's own 3-D points
    @staticmethod
    def project(points3d, cam_intr):
        hom_2d = np.array(cam_intr).dot(np.asarray(points3d).transpose()).transpose()
        return (hom_2d / hom_2d[:, 2:])[:, :2].astype(np.float32)

    def get_joints2d(self, idx):
        return self.project(self.get_joints3d(idx), self.get_camintr(idx))

    def get_objverts2d(self, idx):
        return self.project(self.get_obj_verts_trans(idx), self.get_camintr(idx))

    def get_hand_verts2d(self, idx):
        return self.project(self.get_hand_verts3d(idx), self.get_camintr(idx))

    def get_dist_idx(self, idx, dist=1):
        """Closest annotated frame `dist` steps ahead (> 0) or behind (< 0) inside the same scene."""
        other = idx ^ 1 if dist != 0 else idx
        return other, abs(other - idx)
