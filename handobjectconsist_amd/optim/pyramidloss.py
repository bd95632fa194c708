"""Photometric criterion -- drop-in for meshreg/optim/pyramidloss.py.

The two criteria the reference's trainer offers with ``level_nb=1`` are on the hot path:
``PyramidCriterion('l1')`` (warpreg.py:34, trainmeshwarp.py ``--consist_criterion l1``, the
default) and ``PyramidCriterion('l2')`` (``--consist_criterion l2``).  ``imgflowarp.pair_consist``,
``opticalflow.flow_pair_loss`` and ``warpbranch.forward`` recognise them
(``imgflowarp._fused_criterion``) and run the fused HIP kernels with the matching
MR_CRITERION_* instantiation (|res| or res * res per channel, then the same per-sample masked
mean); ``compute`` below is what the composed path runs.  ``ssim`` and ``level_nb > 1`` need
kornia's SSIM / ScalePyramid (third-party, never enabled by any reference script): out of scope,
they raise NotImplementedError instead of silently computing something else."""
import torch

from handobjectconsist_amd.optim import lossutils


class PyramidCriterion:
    def __init__(self, criterion, geom_weight=1, level_nb=1):
        self.level_nb = level_nb
        if criterion == "l2":
            self.criterion = torch.nn.MSELoss(reduction="none")
        elif criterion == "l1":
            self.criterion = torch.nn.L1Loss(reduction="none")
        elif criterion == "ssim":
            raise NotImplementedError("ssim criterion needs kornia (out of scope, see DESIGN.md)")
        else:
            raise ValueError(f"{criterion} not in [l2, l1, ssim]")
        if level_nb != 1:
            raise NotImplementedError("level_nb > 1 needs kornia.ScalePyramid (out of scope, see DESIGN.md)")
        self.geom_weight = geom_weight

    def compute(self, inp, target, mask=None):
        """reference pyramidloss.py:56-62 (level_nb == 1 branch)."""
        diff = self.criterion(inp, target)
        losses = lossutils.batch_masked_mean_loss(diff, mask)
        return [inp], [target], losses, [diff], [mask]
