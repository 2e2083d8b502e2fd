"""``MaskReconLoss`` of the box2mask path (reference ``models/mask_losses.py:12-27``) on the HIP loss kernel."""
import torch.nn as nn

from .. import ops

IGNORE_INDEX = 255


class MaskReconLoss(nn.Module):
    """``NLLLoss2d(ignore_index=255)`` of channel log-probabilities against an id map in which every position with
    ``gt_mask < 0.5`` is ignored: the mean of ``-log p[label]`` over the positions inside the mask.  The reference rewrites
    those labels to 255 on the host and calls the torch loss; here the mask is read by the kernel (``him_masked_nll_*``).

    ``boundary_weight`` A > 0 (an addition of this build): every valid position weighs
    ``1 + A * exp(-d^2 / (2 boundary_sigma^2))``, d its distance to the nearest class boundary of the ground-truth map, and
    the loss is the weighted mean (``ops.boundary_weighted_nll``).  With A = 0 the call is ``ops.masked_nll``, as before."""

    def __init__(self, use_nll=True, boundary_weight=0.0, boundary_sigma=5.0):
        super().__init__()
        assert use_nll
        self.boundary_weight, self.boundary_sigma = float(boundary_weight), float(boundary_sigma)
        if not self.boundary_weight >= 0.0 or not self.boundary_sigma > 0.0:
            raise ValueError('MaskReconLoss: boundary_weight >= 0 and boundary_sigma > 0, got %r and %r'
                             % (boundary_weight, boundary_sigma))

    def forward(self, pred_logit, gt_label_, gt_mask, dist2=None):
        """pred_logit (B,C,H,W) log-probabilities, gt_label_ (B,H,W) or (B,1,H,W) ids (long or float), gt_mask (B,1,H,W)."""
        label = gt_label_.float()
        if label.dim() == 3:
            label = label.unsqueeze(1)
        if self.boundary_weight > 0.0:
            return ops.boundary_weighted_nll(pred_logit, label.contiguous(), gt_mask, self.boundary_weight,
                                             self.boundary_sigma, dist2)
        return ops.masked_nll(pred_logit, label.contiguous(), gt_mask)
