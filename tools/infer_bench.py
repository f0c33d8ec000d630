"""GuideDepth inference at the NYU sizes (frames 480x640; model at 'half' 240x320 and at
'full' 480x640) on synthetic frames and random weights, four comparisons:

  forward   eager model(x) under no_grad against the replayed graph (CompiledForward),
            batch 1 and 2, with the graph's kernel-node count and replay time per node;
  front     functional.infer_prep on uint8 frames against the composition of the existing
            ops (permute / float / div(255), flip, cat, bilinear_resize), each with its
            own host-to-device copy (uint8 frame, or the float image) and without;
  back      functional.depth_from_inverse against reciprocal * max / clamp /
            bilinear_resize;
  e2e       Inference_Engine.predict(uint8 frame) at batch 1 against the eager
            composition, and engine_evaluate() against Evaluater(batch_size=1) on
            device-resident images, images/s.

Every arm is warmed up, the two arms of a comparison alternate within each repeat, times
are host time around work that ends in a device synchronise, and each figure is the
median with the min-max spread over the repeats.  Ends with one JSON line.

--antialias: the front and e2e comparisons with the antialiased downscale on both arms
(infer_prep / bilinear_resize(..., antialias=True), Inference_Engine and Evaluater made with
antialias=True); tools/aa_bench.py measures that kernel on its own.

  python tools/infer_bench.py [--repeats 7] [--iters 20] [--images 64] [--antialias]
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import tempfile
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

MAXD = 10.0
FRAME = (480, 640)
SIZES = {"half": (240, 320), "full": (480, 640)}


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def compare(arms, repeats, iters, scale=1e3):
    """{name: spread} of the arms' time per call (ms by default), alternating within a repeat."""
    for fn in arms.values():
        timed(fn, 3)
    times = {k: [] for k in arms}
    for _ in range(repeats):
        for k, fn in arms.items():
            times[k].append(timed(fn, iters) * scale)
    return {k: spread(v) for k, v in times.items()}


def verdict(r, old, new):
    """Whether `new` improves on `old` by more than old's own min-max spread."""
    gain = r[old]["median"] - r[new]["median"]
    noise = r[old]["max"] - r[old]["min"]
    return {"gain": gain, "old_spread": noise, "beyond_spread": gain > noise}


def show(title, r, unit="ms"):
    for k, s in r.items():
        if isinstance(s, dict) and "median" in s:
            print(f"{title:34s} {k:12s}: {s['median']:9.3f} {unit} (min {s['min']:.3f}, "
                  f"max {s['max']:.3f})", flush=True)


def to_tensor_dev(frames):
    return frames.permute(0, 3, 1, 2).float().div(255)


def bench_forward(model, a):
    from monocular_depth_estimation_amd.GuideDepth.inference import CompiledForward
    cf = CompiledForward(model)
    out = {}
    for res, (h, w) in SIZES.items():
        for b in (1, 2):
            x = torch.rand((b, 3, h, w), device="cuda")

            def eager(x=x):
                with torch.no_grad():
                    return model(x)

            r = compare({"eager": eager, "replay": lambda x=x: cf(x)}, a.repeats, a.iters)
            nodes = cf.node_counts((b, 3, h, w))
            r["kernel_nodes"] = nodes["kernel"]
            r["total_nodes"] = nodes["total"]
            r["replay_us_per_kernel_node"] = 1e3 * r["replay"]["median"] / nodes["kernel"]
            r["verdict"] = verdict(r, "eager", "replay")
            out[f"{res}_b{b}"] = r
            show(f"forward {res} batch {b}", r)
            print(f"{'':34s} kernel nodes {nodes['kernel']} (total {nodes['total']}), "
                  f"{r['replay_us_per_kernel_node']:.2f} us per node", flush=True)
    cf.close()
    return out


def bench_front(a):
    from monocular_depth_estimation_amd.functional import bilinear_resize, infer_prep
    out = {}
    for res, size in SIZES.items():
        for n in (1,):
            host_u8 = torch.randint(0, 256, (n, *FRAME, 3), dtype=torch.uint8).pin_memory()
            host_f = host_u8.permute(0, 3, 1, 2).float().div(255).contiguous().pin_memory()
            dev_u8 = host_u8.cuda()
            buf = torch.empty((2 * n, 3, *size), device="cuda")

            def composed(img):
                return bilinear_resize(torch.cat([img, torch.flip(img, [3])]), size=size,
                                       antialias=a.antialias)

            arms = {
                "ops+copy": lambda: composed(host_f.cuda(non_blocking=True)),
                "fused+copy": lambda: infer_prep(host_u8.cuda(non_blocking=True), size, 2, out=buf,
                                                 antialias=a.antialias),
                "ops": lambda: composed(to_tensor_dev(dev_u8)),
                "fused": lambda: infer_prep(dev_u8, size, 2, out=buf, antialias=a.antialias),
            }
            r = compare(arms, a.repeats, a.iters, scale=1e6)
            r["verdict_with_copy"] = verdict(r, "ops+copy", "fused+copy")
            r["verdict"] = verdict(r, "ops", "fused")
            out[f"{res}_n{n}"] = r
            show(f"front end {res} n {n}", r, "us")
    return out


def bench_back(a):
    from monocular_depth_estimation_amd.functional import bilinear_resize, depth_from_inverse
    out = {}
    for res, size in SIZES.items():
        inv = 0.3 + 39.7 * torch.rand((1, 1, *size), device="cuda")
        buf = torch.empty((1, 1, *FRAME), device="cuda")

        def composed():
            d = torch.clamp(MAXD / inv, MAXD / 100, MAXD)
            return bilinear_resize(d, size=FRAME) if size != FRAME else d

        r = compare({"ops": composed,
                     "fused": lambda: depth_from_inverse(inv, FRAME, MAXD, out=buf)},
                    a.repeats, a.iters, scale=1e6)
        r["verdict"] = verdict(r, "ops", "fused")
        out[res] = r
        show(f"back end {res}", r, "us")
    return out


def bench_e2e(model, a):
    from monocular_depth_estimation_amd.functional import bilinear_resize
    from monocular_depth_estimation_amd.GuideDepth.evaluate import Evaluater
    from monocular_depth_estimation_amd.GuideDepth.inference import Inference_Engine
    out = {}
    gen = torch.Generator(device="cuda").manual_seed(1)
    frames = torch.randint(0, 256, (a.images, *FRAME, 3), dtype=torch.uint8, device="cuda",
                           generator=gen)
    gts = 0.3 + 9.5 * torch.rand((a.images, 1, *FRAME), device="cuda", generator=gen)
    floats = to_tensor_dev(frames).contiguous()
    host_frame = frames[:1].cpu().pin_memory()
    with tempfile.TemporaryDirectory() as tmp:
        for res, size in SIZES.items():
            args = types.SimpleNamespace(dataset="nyu", resolution=res, eval_mode="alhashim",
                                         save_results=tmp, model="GuideDepth", weights_path=None,
                                         evaluate=False)
            with contextlib.redirect_stdout(io.StringIO()):
                eng = Inference_Engine(args, model=model, antialias=a.antialias)
                ev = Evaluater(args, model=model, batch_size=1, antialias=a.antialias,
                               test_loader=[(floats[i:i + 1], gts[i:i + 1]) for i in range(a.images)])
            eng.test_loader = [(frames[i:i + 1], gts[i:i + 1]) for i in range(a.images)]

            def eager_predict():
                with torch.no_grad():
                    img = to_tensor_dev(host_frame.cuda(non_blocking=True))
                    if size != FRAME:
                        img = bilinear_resize(img, size=size, antialias=a.antialias)
                    d = torch.clamp(MAXD / model(img), MAXD / 100, MAXD)
                    return bilinear_resize(d, size=FRAME) if size != FRAME else d

            r = compare({"eager": eager_predict, "predict": lambda: eng.predict(host_frame)},
                        a.repeats, a.iters)
            r["verdict"] = verdict(r, "eager", "predict")
            out[f"predict_{res}"] = r
            show(f"predict {res} batch 1", r)

            rates = {"Evaluater_b1": [], "engine_evaluate": []}
            with contextlib.redirect_stdout(io.StringIO()):
                ev.evaluate()
                eng.engine_evaluate()
                for _ in range(max(3, a.repeats // 2)):
                    rates["Evaluater_b1"].append(a.images / timed(ev.evaluate, 1))
                    rates["engine_evaluate"].append(a.images / timed(eng.engine_evaluate, 1))
            r = {k: spread(v) for k, v in rates.items()}
            gain = r["engine_evaluate"]["median"] - r["Evaluater_b1"]["median"]
            noise = r["Evaluater_b1"]["max"] - r["Evaluater_b1"]["min"]
            r["verdict"] = {"gain": gain, "old_spread": noise, "beyond_spread": gain > noise}
            out[f"evaluate_{res}"] = r
            show(f"evaluate {res} ({a.images} images)", r, "images/s")
            eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--antialias", action="store_true",
                    help="the antialiased downscale in the front and e2e comparisons")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "infer_bench needs a ROCm GPU"
    from monocular_depth_estimation_amd.GuideDepth.model.GuideDepth import GuideDepth
    torch.manual_seed(0)
    model = GuideDepth(pretrained=False).to("cuda").eval()
    res = {"device": torch.cuda.get_device_name(0), "frame": FRAME, "sizes": SIZES,
           "repeats": a.repeats, "iters": a.iters, "images": a.images,
           "antialias": a.antialias}
    res["forward_ms"] = bench_forward(model, a)
    res["front_us"] = bench_front(a)
    res["back_us"] = bench_back(a)
    res["e2e"] = bench_e2e(model, a)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
