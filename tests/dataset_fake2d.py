"""``tests/dataset_fake.FakePoseDataset`` with the three 2-D accessors of the reference's dataset classes, for the 2-D fixture
(tests/golden/chain_dataset2d.npz) -- INPUTS only, written out here and not inherited, so that the fixture does not depend on the
package's own accessors: ``get_objverts2d`` and ``get_hand_verts2d`` in ho3dv2.py's form (:350-354, 454-458: ``project`` on the
accessor's own 3-D points, float32), ``get_joints2d`` as ANNOTATED pixels in float64 (fhbhands.py:429-432 hands out float64
annotations): the host path transforms the array it was given and casts afterwards, as the reference does."""
import numpy as np

from tests.dataset_fake import CONFIGS, INP_RES, FakePoseDataset  # noqa: F401


def project(points3d, cam_intr):
    hom_2d = np.array(cam_intr).dot(points3d.transpose()).transpose()
    return (hom_2d / hom_2d[:, 2:])[:, :2].astype(np.float32)


class FakePoseDataset2d(FakePoseDataset):
    def get_joints2d(self, idx):
        hom = np.asarray(self.get_camintr(idx), np.float64).dot(np.asarray(self.get_joints3d(idx), np.float64).T).T
        return hom[:, :2] / hom[:, 2:]

    def get_objverts2d(self, idx):
        return project(self.get_obj_verts_trans(idx), self.get_camintr(idx))

    def get_hand_verts2d(self, idx):
        return project(self.get_hand_verts3d(idx), self.get_camintr(idx))
