"""Deployment of a trained GuideDepth checkpoint (src/GuideDepth/inference.py) on MI355X.

The reference freezes the PyTorch module into a TensorRT engine (torch2trt),
times it at batch 1 against the eager module, evaluates it on raw test frames
and writes `{dataset}_{resolution}_{model}.txt`.  Here the frozen engine is a
replayed hipGraph:

    uint8 frame [n, H, W, 3]
      -- one H2D copy into a static buffer --
      infer_prep          to_tensor, (flip,) bilinear resize to the model resolution
                          (plain, or antialiased with antialias=True: one launch either way)
      model               the eval-mode forward, every launch captured
      depth_from_inverse  inverse_depth_norm + bilinear upscale to the frame
    depth [n, 1, H, W] metres

`CompiledForward` is the torch2trt replacement: the forward (or the whole path
above) captured once per input shape with _abi.capture_graph and replayed, so a
batch-1 forward costs one graph launch instead of a few hundred kernel launches
from Python.  `Inference_Engine` is the reference's class on top of it, with the
reference's tables, helpers, speed tests, evaluation loop and results file.

What differs from the reference

  * No `.engine` file is written: a hipGraph cannot be serialised.  The engine
    is rebuilt from the checkpoint in the constructor (a second or two).
  * `engine_speedtest` / `engine_evaluate` are the reference's
    `tensorRT_speedtest` / `tensorRT_evaluate`; the old names are aliases, so
    scripts written against the reference run.
  * The evaluation loop is GuideDepth.evaluate.Evaluater's in 'alhashim' mode (the
    same loop as inference.py:208-280): both views through one forward, the tail
    in functional.eval_pair_sums, one device-to-host read at the end.  Frames
    that arrive as uint8 go through functional.infer_prep.
  * `run_evaluation()` runs from the constructor only when args.evaluate is set
    and a test_loader was given (the reference would crash without a loader);
    the reference's data.datasets / data.transforms modules are not part of the
    reference tree, so `test_loader` is any iterable of (image, gt): image uint8
    [B, H, W, 3] / [H, W, 3] or float32 [B, 3, H, W] in [0, 1], gt [B, 1, H, W]
    metres.
  * The reference's transforms.Resize antialiases float tensors from torchvision
    0.17 on.  Inference_Engine(..., antialias=True) (or args.antialias = True)
    gives that filter in the same single front-end launch (functional.infer_prep
    on csrc/aa.hip); the default stays the plain bilinear filter of the
    torchvision the reference was written against.
  * save_image_results (matplotlib figures of selected images) is left out, as in
    GuideDepth.evaluate.
  * fp16_mode has no counterpart; amp="bf16" replays the autocast forward.
"""
from __future__ import annotations

import argparse
import os
import time
import types

import torch

from .. import _abi
from .. import functional as F
from .evaluate import Evaluater
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
    'half': (192, 640)}
resolutions = {
    'nyu': nyu_res,
    'nyu_reduced': nyu_res,
    'kitti': kitti_res}
crops = {
    'kitti': [128, 381, 45, 1196],
    'nyu': [20, 460, 24, 616],
    'nyu_reduced': [20, 460, 24, 616]}

RESULTS_HEADER = 's[PyTorch], s[tensorRT], RMSE,MAE,REL,Lg10,Delta1,Delta2,Delta3\n'


def get_args(argv=None):
    """The reference's command line (inference.py:38-83): same options, same defaults."""
    p = argparse.ArgumentParser(description='GuideDepth inference engine on a ROCm device')
    p.add_argument('--eval', dest='evaluate', action='store_true', default=False,
                   help='time and evaluate the engine (needs a test loader)')
    p.add_argument('--test_path', type=str, help='where the test split lives')
    p.add_argument('--dataset', type=str, default='kitti', choices=sorted(max_depths),
                   help='selects max depth, resolutions and crop')
    p.add_argument('--resolution', type=str, default='half', choices=['full', 'half'],
                   help='model input resolution (a key of the dataset\'s table)')
    p.add_argument('--model', type=str, default='UpDepth',
                   help='a name model.loader.model_builder knows')
    p.add_argument('--weights_path', type=str, help='checkpoint to load')
    p.add_argument('--save_results', type=str, default='./results',
                   help='directory of {dataset}_{resolution}_{model}.txt')
    p.add_argument('--num_workers', type=int, default=1, help='loader workers')
    return p.parse_args(argv)


def results_line(average, engine_speed, pyTorch_speed) -> str:
    """The contents of {dataset}_{resolution}_{model}.txt (inference.py:284-297)."""
    return (RESULTS_HEADER +
            '{pyTorch_speed:.3f}'
            ',{engine_speed:.3f}'
            ',{average.rmse:.3f}'
            ',{average.mae:.3f}'
            ',{average.absrel:.3f}'
            ',{average.lg10:.3f}'
            ',{average.delta1:.3f}'
            ',{average.delta2:.3f}'
            ',{average.delta3:.3f}'.format(average=average, engine_speed=engine_speed,
                                           pyTorch_speed=pyTorch_speed))


def _autocast(amp: str, device):
    if amp not in ("", "fp32", "bf16"):
        raise ValueError(f"unsupported amp {amp!r} (fp32 or bf16)")
    return torch.autocast(device.type, dtype=torch.bfloat16, enabled=amp == "bf16",
                          cache_enabled=False)


class Pipeline:
    """One captured frame-to-depth graph over static buffers (CompiledForward.
    compile_pipeline): write `frames`, replay(), read `depth` (and `inv`, the
    network's output for every view).  The next replay overwrites them."""

    def __init__(self, graph, frames, net_in, inv, depth):
        self.graph, self.frames, self.net_in, self.inv, self.depth = graph, frames, net_in, inv, depth

    def replay(self):
        self.graph.replay()
        return self.depth


class CompiledForward:
    """model's eval-mode forward as a replayed hipGraph: the torch2trt replacement.

    CompiledForward(model, amp="") puts the model in eval mode.  One graph per
    input shape (b, 3, h, w), compiled on first use: two eager forwards on a side
    stream (the libraries pick their kernels, the allocator settles, the model's
    filter-pack tables are registered), then one capture of the forward from a
    static input buffer into a private memory pool, its memset nodes repaired
    (_abi.capture_graph).

    __call__(x) copies x into the static input, replays the graph on the current
    stream and returns the STATIC output tensor: the next call with the same
    shape overwrites it, so clone() what must outlive that call.  No autograd.

    Contracts
      * Weights and buffers are read at replay time: the filter transforms and
        packs are the table launches inside nn.convbf_pack_scope, captured with
        the forward.  An in-place update (p.mul_(...), load_state_dict, a changed
        running_mean) is seen by the next replay.
      * Replacing a Parameter or buffer OBJECT (model.conv.weight = Parameter(...),
        .to(), .half()) leaves the graphs reading the old memory: call
        recompile().
      * A model put back in training mode is refused (BatchNorm would update its
        statistics inside the replay).
      * amp="bf16": capture under torch.autocast(bfloat16, cache_enabled=False);
        the replay equals the eager forward under the same autocast.
      * A replay runs the kernels the eager forward launched while the shape was
        compiled, so it equals the eager forward as far as that equals itself.
        With the library's default convolution solvers it does not, in the last
        bits, at the small deep-layer shapes; with
        torch.backends.cudnn.deterministic = True set while a shape is compiled
        the graph holds the deterministic kernels, and replay and eager (under
        the same flag) agree bit for bit.
    close() frees the graphs and their pools."""

    def __init__(self, model, amp: str = ""):
        if not torch.cuda.is_available():
            raise RuntimeError("CompiledForward runs on a ROCm device; there is no CPU fallback")
        self.model = model.eval()
        self.amp = amp
        p = next(model.parameters(), None)
        self.device = p.device if p is not None else torch.device('cuda', torch.cuda.current_device())
        if self.device.type != "cuda":
            raise RuntimeError(f"CompiledForward needs the model on a ROCm device, got {self.device}")
        _autocast(amp, self.device)  # validates amp
        self.graphs = {}     # (b, 3, h, w) -> (graph, static input, static output)
        self.pipelines = {}  # compile_pipeline's key -> Pipeline
        self.stream = torch.cuda.Stream(device=self.device)        # capture stream
        self.eager_stream = torch.cuda.Stream(device=self.device)  # warm-up forwards
        self.memsets_replaced = 0

    # ---------------------------------------------------------------- compile
    def _check_mode(self):
        if self.model.training:
            raise RuntimeError("CompiledForward replays the eval-mode forward, but the model is in "
                               "training mode: call model.eval() (a captured train-mode BatchNorm "
                               "would update its running statistics on every replay)")

    def _capture(self, body, warm):
        """Two eager `warm()` on the side stream, then `body()` captured; returns
        (graph, body's result)."""
        self._check_mode()
        cur = torch.cuda.current_stream(self.device)
        self.eager_stream.wait_stream(cur)
        with torch.no_grad(), _autocast(self.amp, self.device):
            with torch.cuda.stream(self.eager_stream):
                for _ in range(2):
                    warm()
            cur.wait_stream(self.eager_stream)
            torch.cuda.synchronize(self.device)
            graph, out, n = _abi.capture_graph(body, self.stream)
        self.memsets_replaced += n
        return graph, out

    def _compile(self, shape):
        static_in = torch.zeros(shape, dtype=torch.float32, device=self.device)
        graph, static_out = self._capture(lambda: self.model(static_in),
                                          lambda: self.model(static_in))
        self.graphs[shape] = (graph, static_in, static_out)
        return self.graphs[shape]

    def compile_pipeline(self, frame_shape, frame_dtype, size, out_size, max_depth, views=1,
                         antialias=False):
        """The whole path as ONE graph over static buffers: infer_prep of `views`
        views -> model -> depth_from_inverse of view 0.  frame_shape / frame_dtype:
        uint8 (n, H, W, 3) or float32 (n, 3, H, W); size: the model resolution;
        out_size: the depth map's; antialias: infer_prep's filter (still one
        node).  Returns the Pipeline (kept; the same arguments return the same
        one)."""
        key = (tuple(frame_shape), frame_dtype, tuple(size), tuple(out_size), float(max_depth),
               int(views), bool(antialias))
        if key in self.pipelines:
            return self.pipelines[key]
        frames = torch.zeros(key[0], dtype=frame_dtype, device=self.device)
        n = key[0][0]
        net_in = torch.empty((views * n, 3, *key[2]), dtype=torch.float32, device=self.device)
        depth = torch.empty((n, 1, *key[3]), dtype=torch.float32, device=self.device)

        def body():
            F.infer_prep(frames, key[2], views=views, out=net_in, antialias=key[6])
            inv = self.model(net_in)
            F.depth_from_inverse(inv[:n].float(), key[3], max_depth, out=depth)
            return inv

        graph, inv = self._capture(body, body)
        self.pipelines[key] = Pipeline(graph, frames, net_in, inv, depth)
        return self.pipelines[key]

    # ------------------------------------------------------------------ replay
    def __call__(self, x):
        """model(x) from the replayed graph of x's shape.  Returns the graph's static
        output: the next call with this shape overwrites it."""
        self._check_mode()
        shape = tuple(x.shape)
        entry = self.graphs.get(shape)
        if entry is None:
            if len(shape) != 4 or x.dtype != torch.float32:
                raise ValueError(f"expected a float32 [b, 3, h, w] input, got {x.dtype} "
                                 f"{shape}")
            entry = self._compile(shape)
        graph, static_in, static_out = entry
        if x is not static_in:  # a caller may have written static_input(shape) itself
            static_in.copy_(x, non_blocking=True)
        graph.replay()
        return static_out

    def static_input(self, shape):
        """The static input buffer of `shape`'s graph (compiled if need be), for a
        producer that writes it in place (functional.infer_prep(..., out=)); pass
        that same tensor to __call__ and no copy is made."""
        self._check_mode()
        shape = tuple(int(s) for s in shape)
        entry = self.graphs.get(shape) or self._compile(shape)
        return entry[1]

    def node_counts(self, shape) -> dict:
        """Node census of the graph compiled for `shape` (after the memset repair):
        {'total', 'kernel', 'memcpy', 'memset', 'event', 'other'}."""
        entry = self.graphs.get(tuple(shape))
        if entry is None:
            raise KeyError(f"no graph compiled for input shape {tuple(shape)}")
        return dict(entry[0].node_counts)

    def recompile(self):
        """Drop every graph; each shape is captured again on its next use.  Needed
        after a Parameter or buffer object of the model was replaced."""
        self.close()

    def close(self):
        """Drain the device and free the captured graphs."""
        if not self.graphs and not self.pipelines:
            return
        torch.cuda.synchronize(self.device)
        for graph, _, _ in self.graphs.values():
            graph.reset()
        for pipe in self.pipelines.values():
            pipe.graph.reset()
        self.graphs, self.pipelines = {}, {}
        torch.cuda.synchronize(self.device)


class _EngineEvaluater(Evaluater):
    """Evaluater's 'alhashim' loop with the engine in place of the eager module: uint8
    (or float) frames through infer_prep, both views through the replayed forward."""

    def __init__(self, engine):
        # the fields Evaluater's loop reads; nothing is loaded or printed twice
        self.dataset = engine.dataset
        self.maxDepth = engine.maxDepth
        self.resolution = engine.resolution
        self.crop = list(engine.crop)
        self.eval_mode = 'alhashim'
        self.device = engine.device
        self.model = engine.model
        self.test_loader = engine.test_loader
        self.batch_size = 1
        self.result_dir = engine.result_dir
        self.engine = engine
        self.antialias = getattr(engine, 'antialias', False)

    def _both_views(self, image):
        if image.dtype != torch.uint8:
            image = image.to(dtype=torch.float32)
        image = image.to(self.device, non_blocking=True)
        # straight into the graph's static input: the forward of the previous batch
        # and its eval_pair_sums are ahead of this launch on the stream
        buf = self.engine.trt_model.static_input((2 * image.shape[0], 3, *self.resolution))
        return F.infer_prep(image, self.resolution, views=2, out=buf, antialias=self.antialias)

    def _forward_pair(self, both):
        b = both.shape[0] // 2
        out = self.engine.trt_model(both)
        return out[:b], out[b:]

    def save_results(self, average):
        pass  # Inference_Engine.save_results writes the engine's file


class Inference_Engine():
    """Inference_Engine(args, model=None, test_loader=None, antialias=None) -- see the module
    docstring.

    args: dataset ('nyu', 'nyu_reduced', 'kitti'), resolution ('full' / 'half', or
    an (h, w) pair), model, weights_path (when `model` is None), save_results (the
    results directory), evaluate.  Optional: amp ('' or 'bf16').
    antialias: infer_prep's filter in predict() and engine_evaluate(); None takes
    getattr(args, 'antialias', False).  get_args() has the reference's options only:
    give the flag here or set it on the namespace."""

    def __init__(self, args, model=None, test_loader=None, antialias=None):
        self.antialias = bool(getattr(args, 'antialias', False) if antialias is None else antialias)
        self.dataset = args.dataset
        self.maxDepth = max_depths[args.dataset]
        self.res_dict = resolutions[args.dataset]
        res = args.resolution
        self.resolution = self.res_dict[res] if isinstance(res, str) else (int(res[0]), int(res[1]))
        self.resolution_keyword = args.resolution
        print('Resolution for Eval: {}'.format(self.resolution))
        print('Maximum Depth of Dataset: {}'.format(self.maxDepth))
        self.crop = crops[args.dataset]

        self.result_dir = args.save_results
        if not os.path.isdir(self.result_dir):
            os.makedirs(self.result_dir)
        name = res if isinstance(res, str) else '{}x{}'.format(*self.resolution)
        self.results_filename = '{}_{}_{}'.format(args.dataset, name, args.model)

        if not torch.cuda.is_available():
            raise RuntimeError("Inference_Engine runs on a ROCm device; there is no CPU fallback")
        self.device = torch.device('cuda', torch.cuda.current_device())
        if model is None:
            model = loader.load_model(args.model, args.weights_path, device=self.device)
        self.model = model.eval().to(self.device)
        self.test_loader = test_loader
        self.visualize_images = []

        print('[engine] Capturing the forward into a hipGraph')
        self.trt_model = CompiledForward(self.model, amp=getattr(args, 'amp', '') or '')
        self.trt_model(torch.ones([1, 3, *self.resolution], device=self.device))
        print('[engine] Model compiled\n')

        if getattr(args, 'evaluate', False) and test_loader is not None:
            self.run_evaluation()

    def run_evaluation(self):
        speed_pyTorch = self.pyTorch_speedtest()
        speed_engine = self.engine_speedtest()
        average = self.engine_evaluate()
        self.save_results(average, speed_engine, speed_pyTorch)

    # ------------------------------------------------------------- speed tests
    def _speedtest(self, fn, tag, num_test_runs):
        torch.cuda.empty_cache()
        times = 0.0
        warm_up_runs = 10
        for i in range(num_test_runs + warm_up_runs):
            if i == warm_up_runs:
                times = 0.0
            x = torch.randn([1, 3, *self.resolution]).to(self.device)
            torch.cuda.synchronize()  # the transfer is not timed
            t0 = time.time()
            fn(x)
            torch.cuda.synchronize()
            times += time.time() - t0
        times = times / num_test_runs
        print('[{}] Runtime: {}s'.format(tag, times))
        print('[{}] FPS: {}\n'.format(tag, 1 / times))
        return times

    def pyTorch_speedtest(self, num_test_runs=200):
        """Seconds per eager model(x) at batch 1 (inference.py:141-161), under no_grad
        and the engine's autocast."""
        def eager(x):
            with torch.no_grad(), _autocast(self.trt_model.amp, self.device):
                return self.model(x)
        return self._speedtest(eager, 'PyTorch', num_test_runs)

    def engine_speedtest(self, num_test_runs=200):
        """Seconds per replayed forward at batch 1 (inference.py:165-185)."""
        return self._speedtest(self.trt_model, 'engine', num_test_runs)

    tensorRT_speedtest = engine_speedtest

    # ----------------------------------------------------------------- predict
    def predict(self, frames):
        """Metric depth [n, 1, H, W] (metres, a copy) at the frames' resolution for
        uint8 [n, H, W, 3] (or one [H, W, 3]) or float32 [n, 3, H, W] frames on the
        host or the device: one copy into the pipeline's static buffer, one replay."""
        if frames.dtype == torch.uint8:
            if frames.dim() == 3:
                frames = frames[None]
            if frames.dim() != 4 or frames.shape[3] != 3:
                raise ValueError(f"uint8 frames are [n, H, W, 3], got {tuple(frames.shape)}")
            out_size = tuple(frames.shape[1:3])
        elif frames.dtype == torch.float32 and frames.dim() == 4 and frames.shape[1] == 3:
            out_size = tuple(frames.shape[2:])
        else:
            raise TypeError(f"expected uint8 [n, H, W, 3] or float32 [n, 3, H, W] frames, got "
                            f"{frames.dtype} {tuple(frames.shape)}")
        pipe = self.trt_model.compile_pipeline(tuple(frames.shape), frames.dtype, self.resolution,
                                               out_size, self.maxDepth, views=1,
                                               antialias=self.antialias)
        self.trt_model._check_mode()
        pipe.frames.copy_(frames, non_blocking=True)
        return pipe.replay().clone()

    # ---------------------------------------------------------------- evaluate
    def engine_evaluate(self):
        """The reference's loop (inference.py:208-280) on the compiled forward; returns
        the averaged Result."""
        if self.test_loader is None:
            raise ValueError("engine_evaluate needs a test_loader: an iterable of (image uint8 "
                             "[B,H,W,3] or float [B,3,H,W] in [0,1], gt [B,1,H,W] metres)")
        torch.cuda.empty_cache()
        return _EngineEvaluater(self).evaluate()

    tensorRT_evaluate = engine_evaluate

    def save_results(self, average, engine_speed, pyTorch_speed):
        file_path = os.path.join(self.result_dir, '{}.txt'.format(self.results_filename))
        with open(file_path, 'w') as f:
            f.write(results_line(average, engine_speed, pyTorch_speed))

    def inverse_depth_norm(self, depth):
        depth = self.maxDepth / depth
        depth = torch.clamp(depth, self.maxDepth / 100, self.maxDepth)
        return depth

    def depth_norm(self, depth):
        depth = torch.clamp(depth, self.maxDepth / 100, self.maxDepth)
        depth = self.maxDepth / depth
        return depth

    def unpack_and_move(self, data):
        """(image, gt) on the engine's device from an (image, gt) pair or an
        {'image', 'depth'} dict.  The reference prints and returns None for anything
        else; a library must not hide that, so this raises TypeError."""
        if isinstance(data, dict):
            data = (data['image'], data['depth'])
        elif not isinstance(data, (tuple, list)):
            raise TypeError(f"expected an (image, gt) pair or an image/depth dict, got {type(data)}")
        return tuple(t.to(self.device, non_blocking=True) for t in data[:2])

    def close(self):
        self.trt_model.close()


class Dict2Obj(types.SimpleNamespace):
    """Attribute access to a dict of arguments (inference.py:374-377)."""

    def __init__(self, dictionary):
        super().__init__(**dictionary)


if __name__ == '__main__':
    args = get_args()
    print(args)
    engine = Inference_Engine(args)
