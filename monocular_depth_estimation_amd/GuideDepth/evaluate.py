"""Evaluation of a trained GuideDepth checkpoint (src/GuideDepth/evaluate.py) on MI355X.

`Evaluater` keeps the reference's interface (args, evaluate(), save_results(),
inverse_depth_norm(), depth_norm(), the tables below) and its numbers: per test
image the image and its horizontal flip are predicted, both predictions are
turned into metres, upscaled to the ground-truth resolution, cropped and
measured against the ground truth, and the per-view Results are averaged in the
reference's order.

What runs differently from evaluate.py:84-142

  * both views of a batch go through ONE forward, cat([image, flip(image)])
    (eval-mode BatchNorm is per-sample, so a sample's output does not depend on
    its batch): `predict`;
  * everything between the network and the metrics -- flip of gt,
    inverse_depth_norm, the bilinear upscale, the crop, Result.evaluate of both
    views -- is one HIP pass, functional.eval_pair_sums, that reads each
    ground-truth pixel once and writes 2 x 16 doubles per image into a device
    buffer; the host reads that buffer once, after the loop.

The downscale of 'alhashim' mode

  The reference resizes the image with torchvision's transforms.Resize.  The
  torchvision it was written against resized tensors with a plain bilinear
  filter; torchvision >= 0.17 antialiases them by default
  (F.interpolate(..., mode='bilinear', antialias=True)).  Both are here:
  Evaluater(..., antialias=False), the default, is the plain filter
  (functional.bilinear_resize); antialias=True (or args.antialias = True) is
  the antialiased one, functional.bilinear_resize(..., antialias=True) on
  csrc/aa.hip, for checkpoints trained or scored with the reference on a
  current install.  The upscale of the prediction to the ground truth is the
  same either way: it is a pure upscale, where the antialiased filter has
  support 1 and is the bilinear one up to the last bit.

Not implemented

  * the reference's data.datasets / data.transforms modules are not part of the
    reference tree, so there is no built-in test loader: `test_loader` is any
    iterable of (image [B, 3, H, W] float32 in [0, 1], gt [B, 1, H, W] float32
    metres) on the CPU or the GPU.  Evaluater re-batches it to `batch_size`.
  * save_image_results (matplotlib figures of selected images).
"""
from __future__ import annotations

import os
import time

import numpy as np
import torch

from .. import functional as F
from .metrics import AverageMeter, Result
from .model import loader

max_depths = {
    'kitti': 80.0,
    'nyu': 10.0,
    'nyu_reduced': 10.0,
}
nyu_res = {
    'full': (480, 640),
    'half': (240, 320),
    'mini': (224, 224)}
kitti_res = {
    'full': (384, 1280),
    'tu_small': (128, 416),
    'tu_big': (228, 912),
    'half': (192, 640)}
resolutions = {
    'nyu': nyu_res,
    'nyu_reduced': nyu_res,
    'kitti': kitti_res}
crops = {
    'kitti': [128, 381, 45, 1196],
    'nyu': [20, 460, 24, 616],
    'nyu_reduced': [20, 460, 24, 616]}

_CHUNK = 1024  # images per block of the device sums buffer


def kitti_crop(gt_height: int, gt_width: int) -> np.ndarray:
    """The KITTI evaluation crop for a ground-truth shape (evaluate.py:121-124)."""
    return np.array([0.3324324 * gt_height, 0.91351351 * gt_height,
                     0.0359477 * gt_width, 0.96405229 * gt_width]).astype(np.int32)


def results_text(average) -> str:
    """The contents of results.txt for an averaged Result (evaluate.py:162-171)."""
    return ('RMSE,MAE,REL, RMSE_log,Lg10,Delta1,Delta2,Delta3\n'
            '{average.rmse:.3f}'
            ',{average.mae:.3f}'
            ',{average.absrel:.3f}'
            ',{average.rmse_log:.3f}'
            ',{average.lg10:.3f}'
            ',{average.delta1:.3f}'
            ',{average.delta2:.3f}'
            ',{average.delta3:.3f}'.format(average=average))


class Evaluater():
    """Evaluater(args, model=None, test_loader=None, batch_size=1, antialias=None) -- see the
    module docstring.

    args: dataset ('nyu', 'nyu_reduced', 'kitti'), resolution (a key of the
    dataset's table, or an (h, w) pair), eval_mode ('alhashim': predict at
    `resolution`, upscale, crop; anything else: predict at the ground-truth
    resolution, no crop), save_results (directory of results.txt), and -- when
    `model` is None -- model / weights_path for model.loader.load_model.
    antialias: the downscale's filter; None takes getattr(args, 'antialias', False).
    The upscale to the ground truth does not depend on it (a pure upscale: the
    antialiased filter is the bilinear one there, up to the last bit)."""

    def __init__(self, args, model=None, test_loader=None, batch_size=1, antialias=None):
        self.antialias = bool(getattr(args, 'antialias', False) if antialias is None else antialias)
        self.dataset = args.dataset
        self.maxDepth = max_depths[args.dataset]
        self.res_dict = resolutions[args.dataset]
        res = args.resolution
        self.resolution = self.res_dict[res] if isinstance(res, str) else (int(res[0]), int(res[1]))
        print('Resolution for Eval: {}'.format(self.resolution))
        self.resolution_keyword = args.resolution
        print('Maximum Depth of Dataset: {}'.format(self.maxDepth))
        self.crop = crops[args.dataset]
        self.eval_mode = args.eval_mode

        self.result_dir = args.save_results
        if not os.path.isdir(self.result_dir):
            os.makedirs(self.result_dir)

        if not torch.cuda.is_available():
            raise RuntimeError("Evaluater runs on a ROCm device; there is no CPU fallback")
        self.device = torch.device('cuda', torch.cuda.current_device())

        if model is None:
            model = loader.load_model(args.model, args.weights_path, device=self.device)
        self.model = model.to(self.device)
        self.test_loader = test_loader
        self.batch_size = int(batch_size)
        if self.batch_size < 1:
            raise ValueError("batch_size must be at least 1")

    # ------------------------------------------------------------------ pieces
    def downscale_image(self, image):
        """To the model resolution: plain bilinear, or the antialiased filter when the
        Evaluater was made with antialias=True (module docstring)."""
        return F.bilinear_resize(image, size=self.resolution,
                                 antialias=getattr(self, 'antialias', False))

    def predict(self, image, image_flip=None):
        """(inv, inv_flip): the network's output for `image` [B, 3, h, w] and for its
        horizontal flip (image_flip, default torch.flip(image, [3])), from one
        forward of the 2B samples."""
        if image_flip is None:
            image_flip = torch.flip(image, [3])
        return self._forward_pair(torch.cat([image, image_flip]))

    def _forward_pair(self, both):
        b = both.shape[0] // 2
        out = self.model(both)
        return out[:b], out[b:]

    def _both_views(self, image):
        """cat([image, flip(image)]) on the device, at the model resolution in 'alhashim'
        mode, from a host or device batch of the loader (a hook: GuideDepth.inference
        takes uint8 frames here)."""
        image = image.to(self.device, dtype=torch.float32, non_blocking=True)
        both = torch.cat([image, torch.flip(image, [3])])
        if self.eval_mode == 'alhashim':
            both = self.downscale_image(both)
        return both

    def _batches(self):
        """(cat([image, flip(image)]), gt, data_time) with up to batch_size samples, in the
        loader's order.  As in the reference the flip is taken at full resolution and
        both are downscaled ('alhashim'), all within data_time (evaluate.py:93-100)."""
        images, gts, held = [], [], 0
        t0 = time.time()

        def flush():
            nonlocal images, gts, held, t0
            image = torch.cat(images) if len(images) > 1 else images[0]
            gt = torch.cat(gts) if len(gts) > 1 else gts[0]
            gt = gt.to(self.device, dtype=torch.float32, non_blocking=True)
            item = (self._both_views(image), gt, time.time() - t0)
            images, gts, held, t0 = [], [], 0, time.time()
            return item

        for image, gt in self.test_loader:
            if image.dim() == 3:
                image, gt = image.unsqueeze(0), gt.unsqueeze(0)
            if gt.dim() == 3:
                gt = gt.unsqueeze(1)
            for k in range(image.shape[0]):
                im, g = image[k:k + 1], gt[k:k + 1]
                if held and (im.shape != images[0].shape or g.shape != gts[0].shape):
                    yield flush()
                images.append(im)
                gts.append(g)
                held += 1
                if held == self.batch_size:
                    yield flush()
        if held:
            yield flush()

    # ---------------------------------------------------------------- evaluate
    def evaluate(self):
        if self.test_loader is None:
            raise ValueError("Evaluater needs a test_loader: an iterable of (image [B,3,H,W] in "
                             "[0,1], gt [B,1,H,W] metres) batches")
        self.model.eval()
        average_meter = AverageMeter()
        chunks, used = [], 0          # device [<=_CHUNK, 2, 16] float64 blocks of the sums
        per_batch = []                # (images, data_time, start event, end event)
        with torch.no_grad():
            for both, gt, data_time in self._batches():
                b = gt.shape[0]
                crop = None
                if self.eval_mode == 'alhashim':
                    if self.dataset == 'kitti':
                        self.crop = kitti_crop(*gt.shape[-2:])
                    # the reference's slices clip a window that exceeds the map
                    H, W = gt.shape[-2:]
                    crop = [min(int(self.crop[0]), H), min(int(self.crop[1]), H),
                            min(int(self.crop[2]), W), min(int(self.crop[3]), W)]
                if not chunks or used + b > chunks[-1].shape[0]:
                    if chunks:
                        chunks[-1] = chunks[-1][:used]
                    chunks.append(torch.empty((max(_CHUNK, b), 2, 16), dtype=torch.float64,
                                              device=self.device))
                    used = 0
                start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                inv, inv_flip = self._forward_pair(both)
                F.eval_pair_sums(inv, inv_flip, gt, self.maxDepth, crop,
                                 out=chunks[-1][used:used + b])
                end.record()
                used += b
                per_batch.append((b, data_time, start, end))
        if not chunks:
            raise ValueError("the test_loader gave no images")
        chunks[-1] = chunks[-1][:used]
        sums = (torch.cat(chunks) if len(chunks) > 1 else chunks[0]).cpu().tolist()  # the one read

        # the reference's order: image 0 view 0, image 0 view 1, image 1 view 0, ...
        i = 0
        for b, data_time, start, end in per_batch:
            gpu_time = start.elapsed_time(end) / 1000.0 / b
            for _ in range(b):
                for view in (0, 1):
                    average_meter.update(Result().from_sums(sums[i][view]), gpu_time,
                                         data_time / b, 1)
                i += 1

        # Report
        avg = average_meter.average()
        self.save_results(avg)
        print('\n*\n'
              'RMSE={average.rmse:.3f}\n'
              'MAE={average.mae:.3f}\n'
              'Delta1={average.delta1:.3f}\n'
              'Delta2={average.delta2:.3f}\n'
              'Delta3={average.delta3:.3f}\n'
              'REL={average.absrel:.3f}\n'
              'Lg10={average.lg10:.3f}\n'
              't_GPU={time:.3f}\n'.format(
                  average=avg, time=avg.gpu_time))
        return avg

    def save_results(self, average):
        results_file = os.path.join(self.result_dir, 'results.txt')
        with open(results_file, 'w') as f:
            f.write(results_text(average))

    def inverse_depth_norm(self, depth):
        depth = self.maxDepth / depth
        depth = torch.clamp(depth, self.maxDepth / 100, self.maxDepth)
        return depth

    def depth_norm(self, depth):
        depth = torch.clamp(depth, self.maxDepth / 100, self.maxDepth)
        depth = self.maxDepth / depth
        return depth
