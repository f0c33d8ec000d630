"""GuideDepth on MI355X: DDRNet-23-slim encoder + three guided-upsampling blocks.

Drop-in for src/GuideDepth/model/GuideDepth.py:9-57 (constructor, forward,
471 state_dict keys).  The nearest guides (:46-47, one fused pass) and the
three x2 bilinear upsamples (:49, :52, :55) run on the HIP resize kernels.
"""
from __future__ import annotations

from torch import nn

from ...functional import bilinear_resize_x2_slotted, nearest_pyramid
from ...nn import convbf_pack_scope
from .DDRNet_23_slim import DualResNet_Backbone
from .modules import Guided_Upsampling_Block


class GuideDepth(nn.Module):
    def __init__(self, pretrained=True, up_features=[64, 32, 16],  # noqa: B006 (reference signature)
                 inner_features=[64, 32, 16]):
        super().__init__()
        self.feature_extractor = DualResNet_Backbone(pretrained=pretrained,
                                                     features=up_features[0])
        outs = [up_features[1], up_features[2], 1]
        for i in range(3):
            setattr(self, f"up_{i + 1}", Guided_Upsampling_Block(
                in_features=up_features[i], expand_features=inner_features[i],
                out_features=outs[i], kernel_size=3, channel_attention=True,
                guide_features=3, guidance_type="full"))
            # up_3's skip gradient is handed over as (gout, weight), never written
            getattr(self, f"up_{i + 1}").fold_full_res = True

    def forward(self, x):
        with convbf_pack_scope(self, x.device):  # every bf16 filter packed by one launch
            return self._forward(x)

    def _forward(self, x):
        y = self.feature_extractor(x)
        # both nearest guides (:46-47) from one pass over the image
        x_half, x_quarter = nearest_pyramid(x)
        guides = (x_quarter, x_half, x)
        for block, guide in zip((self.up_1, self.up_2, self.up_3), guides):
            # the x2 upsample's backward also takes the skip fusion's gradient
            # of it (GradSlot), so autograd adds no accumulation pass
            y = block(guide, bilinear_resize_x2_slotted(y))
        return y
