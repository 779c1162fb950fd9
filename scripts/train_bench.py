#!/usr/bin/env python
"""WaveNet teacher-forced training step at BASELINE configs[3]: MoL output, 30 layers, per-GPU batch 64 x 8000 samples
(cropped to 7800, datafeeder_wavenet.py:41-47); one process per GPU, gradient all-reduce over RCCL when WORLD_SIZE > 1:
    python scripts/train_bench.py --steps 5
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 scripts/train_bench.py
--width W (32, 64, 128) sets residual_channels = dilation_channels (hparams: 32); --root names another checkout with its own library
(e.g. the parent commit) so that the processes of two builds can alternate on one box; --torch times, instead of the HIP step, the
PyTorch-ROCm float32 autograd step of the same graph on the same batch (tests/torch_train_ref.py: upsample, network_mm, mol_loss,
backward; no optimiser), the composition a user would otherwise run; --log appends the JSON line to a file.
--summarise_wide turns the log and the rocprofv3 kernel statistics of one run per width under --stats_dir/w<W>/
(rocprofv3 --kernel-trace --stats ... -- python scripts/train_bench.py --width W --steps 3) into --out
(default profiles/wavenet_train_wide_bench.txt)."""
import argparse, json, os, sys, time
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64); ap.add_argument("--samples", type=int, default=8000)
ap.add_argument("--layers", type=int, default=30, help="30 as in configs[1]; hparams.py default is 50")
ap.add_argument("--steps", type=int, default=5); ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--width", type=int, default=0); ap.add_argument("--root", default=None); ap.add_argument("--torch", action="store_true")
ap.add_argument("--log", default=None); ap.add_argument("--label", default="")
ap.add_argument("--summarise_wide", action="store_true"); ap.add_argument("--stats_dir", default=None); ap.add_argument("--out", default=None)
args = ap.parse_args()
PEAK_F32_MFMA = 157.3e12                                     # FLOP/s, MI355X: 256 CUs x 4 SIMDs x 64 FLOP/clk x 2.4 GHz


def layer_mfma_flops(W, B, T, dil, ifw=32):
    """FLOPs the wide layer kernels execute on the matrix cores in one step (v_mfma_f32_32x32x2_f32 = 4096 FLOP): per 32-row tile and
    32-channel block, forward 2 W (two taps, filter and gate) + 16 W / 32 (dense) from the layer's offset on; backward, on every tile,
    W / 2 (dZ) and 2 W (dX)"""
    nb, tiles, off, f = W // 32, (T - 1 + 31) // 32, ifw - 1, 0
    for d in dil:
        off += d
        f += B * ((tiles - off // 32) * nb * (2 * W + 16 * nb) + tiles * nb * (W // 2 + 2 * W)) * 4096
    return f


if args.summarise_wide:
    import csv, glob
    med = lambda v: sorted(v)[len(v) // 2]
    rows = [json.loads(l) for l in open(args.log)]
    out = ["WaveNet training step at residual = dilation width 64 and 128 (scripts/train_bench.py --summarise_wide): one step of the 30-layer",
           "model (hop 300, MoL, S = 512), float32; a process per run, the runs of a width alternating on one box", ""]
    for W in (32, 64, 128):
        hip = [r for r in rows if r.get("width") == W and r.get("kind") == "hip" and r.get("build") == "this"]
        par = [r for r in rows if r.get("width") == W and r.get("kind") == "hip" and r.get("build") == "parent"]
        to = [r for r in rows if r.get("width") == W and r.get("kind") == "torch"]
        for name, rr in (("WaveNetTrainer.step (this build)", hip), ("WaveNetTrainer.step (parent build)", par), ("PyTorch float32 autograd step of network_mm", to)):
            for b in sorted({r["batch"] for r in rr}, reverse=True):
                v = [r["ms_per_step"] for r in rr if r["batch"] == b]
                out.append("width %3d  batch %2d x %d  %-44s %s  median %.2f ms" % (W, b, rr[0]["samples"], name, " ".join("%.2f" % x for x in v), med(v)))
        for b in sorted({r["batch"] for r in hip} & {r["batch"] for r in to}, reverse=True):
            h, t = med([r["ms_per_step"] for r in hip if r["batch"] == b]), med([r["ms_per_step"] for r in to if r["batch"] == b])
            out.append("width %3d  batch %2d: the step takes %.2f x the composition's time (%s)" % (W, b, h / t, "faster" if h < t else "SLOWER: a finding, see DESIGN 3c-w"))
        if par and hip:
            a, b = [r["ms_per_step"] for r in par], [r["ms_per_step"] for r in hip]
            out.append("width %3d  this build against the parent: %+.2f %% (the parent's own spread %.2f %%)" % (W, 100 * (med(b) / med(a) - 1), 100 * (max(a) - min(a)) / med(a)))
        f = sorted(glob.glob(os.path.join(args.stats_dir or "", "w%d" % W, "**", "*kernel_stats.csv"), recursive=True))
        if f and hip:
            ks = list(csv.DictReader(open(f[-1])))
            lay = [r for r in ks if "tr_layer_wide" in r["Name"]]
            if lay:
                steps = sum(int(r["Calls"]) for r in lay if "bwd1" in r["Name"]) / 30.0
                lay_ms = sum(float(r["TotalDurationNs"]) for r in lay) / steps / 1e6
                all_ms = sum(float(r["TotalDurationNs"]) for r in ks) / steps / 1e6
                fl = hip[0]["layer_mfma_flops"]
                out.append("width %3d  layer kernels (tr_layer_wide_fwd / bwd1 / bwd2): %.2f ms of %.2f ms kernel time per step (%.1f %%); %.2f TFLOP on the matrix cores -> %.1f TFLOP/s = %.1f %% of the %.1f TFLOP/s f32-MFMA peak" % (
                    W, lay_ms, all_ms, 100 * lay_ms / all_ms, fl / 1e12, fl / lay_ms / 1e9, 100 * fl / (lay_ms * 1e-3) / PEAK_F32_MFMA, PEAK_F32_MFMA / 1e12))
                for r in sorted(ks, key=lambda r: -float(r["TotalDurationNs"]))[:8]:
                    out.append("             %6.2f ms  %5d calls  %s" % (float(r["TotalDurationNs"]) / steps / 1e6, int(int(r["Calls"]) / steps), r["Name"].split("(")[0].replace("void ", "")[:90]))
        out.append("")
    args.out = args.out or os.path.join(HERE, "profiles", "wavenet_train_wide_bench.txt")
    open(args.out, "w").write("\n".join(out) + "\n")
    print("\n".join(out))
    sys.exit(0)

ROOT = os.path.abspath(args.root) if args.root else HERE
sys.path.insert(0, ROOT)
import numpy as np, torch
import twvk_amd
from twvk_amd.wavenet import WaveNetModel
from twvk_amd.train import WaveNetTrainer
rank, world, local = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1)), int(os.environ.get("LOCAL_RANK", 0))
torch.cuda.set_device(local)
if world > 1:
    import torch.distributed as dist
    dist.init_process_group("nccl", device_id=torch.device("cuda", local))
hp = twvk_amd.default_hparams()
hp.dilations = ([1, 2, 4, 8, 16, 32, 64, 128, 256, 512] * 8)[:args.layers]
if args.width:
    hp.residual_channels = hp.dilation_channels = args.width
net = WaveNetModel(batch_size=args.batch, dilations=hp.dilations, filter_width=hp.filter_width, residual_channels=hp.residual_channels,
                   dilation_channels=hp.dilation_channels, skip_channels=hp.skip_channels, quantization_channels=hp.quantization_channels,
                   out_channels=hp.out_channels, use_biases=hp.use_biases, scalar_input=hp.scalar_input,
                   initial_filter_width=hp.initial_filter_width, global_condition_channels=hp.gc_channels,
                   global_condition_cardinality=2, local_condition_channels=hp.num_mels, upsample_factor=hp.upsample_factor,
                   train_mode=True, device="cuda:%d" % local)
rng = np.random.RandomState(100 + rank)
if args.torch:
    # the PyTorch float32 autograd step of the same graph (no optimiser): forward, loss, backward, gradients left in .grad
    sys.path.insert(0, os.path.join(HERE, "tests"))
    import torch_train_ref as R
    from twvk_amd import weights as Wt
    from twvk_amd.train import crop_length
    T = crop_length(args.samples, net.hop_size)
    P = {k: torch.from_numpy(v).cuda().requires_grad_(True) for k, v in Wt.random_tensors(net.specs, seed=0, scale=0.05).items()}
    cfg = dict(dilations=hp.dilations, initial_filter_width=hp.initial_filter_width, use_biases=True, upsample_factor=tuple(hp.upsample_factor))
    audio = torch.from_numpy(((rng.rand(args.batch, T) - 0.5)).astype(np.float32)).cuda()
    lc = torch.from_numpy((rng.randn(args.batch, T // net.hop_size, hp.num_mels) * 0.5).astype(np.float32)).cuda()
    gc = torch.from_numpy(rng.randint(0, 2, args.batch).astype(np.int64)).cuda()

    def torch_step():
        for v in P.values():
            v.grad = None
        loss = R.loss_fn(P, cfg, audio, lc, gc, net=R.network_mm)
        loss.backward()
        return loss
    for _ in range(args.warmup):
        torch_step()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = torch_step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.steps
    rec = {"kind": "torch", "build": "torch", "width": hp.residual_channels, "batch": args.batch, "samples": T, "ms_per_step": dt * 1e3, "loss": float(loss.item()),
           "peak_memory_gb": torch.cuda.max_memory_allocated() / 1e9, "label": args.label}
    print(json.dumps(rec))
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        open(args.log, "a").write(json.dumps(rec) + "\n")
    sys.exit(0)
tr = WaveNetTrainer(net, hp, sample_size=args.samples)
tr.init_weights(seed=0)                                     # identical on every rank
T = tr.sample_size
audio = torch.from_numpy(((rng.rand(args.batch, T) - 0.5)).astype(np.float32)).cuda()
lc = torch.from_numpy((rng.randn(args.batch, T // net.hop_size, hp.num_mels) * 0.5).astype(np.float32)).cuda()
gc = torch.from_numpy(rng.randint(0, 2, args.batch).astype(np.int32)).cuda()
losses = []
for _ in range(args.warmup):
    losses.append(float(tr.step(audio, lc, gc).item()))
torch.cuda.synchronize()
if world > 1:
    dist.barrier()
t0 = time.perf_counter()
for _ in range(args.steps):
    loss = tr.step(audio, lc, gc)
torch.cuda.synchronize()
if world > 1:
    dist.barrier()
dt = time.perf_counter() - t0
losses.append(float(loss.item()))
from twvk_amd.shard import max_over_ranks
dt = max_over_ranks(dt, device="cuda") / args.steps
if rank == 0:
    rec = {"kind": "hip", "build": "parent" if args.root else "this", "width": hp.residual_channels, "batch": args.batch, "samples": T, "ms_per_step": dt * 1e3,
           "loss": losses[-1], "workspace_gb": tr._ws.numel() * 4 / 1e9, "route": tr.route(), "label": args.label,
           "layer_mfma_flops": layer_mfma_flops(hp.residual_channels, args.batch, T, hp.dilations) if hp.residual_channels > 32 else 0}
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        open(args.log, "a").write(json.dumps(rec) + "\n")
    print(json.dumps({"metric": "WaveNet training samples/sec (teacher-forced step, MoL)", "value": world * args.batch * T / dt,
                      "unit": "audio samples/s", "steps_per_s": 1.0 / dt, "ms_per_step": dt * 1e3, "n_gpus": world, "scaling": "weak",
                      "dtype": "f32", "config": {"workload": "configs[3]: train_vocoder.py step, %d layers, per-GPU batch %d x %d samples, "
                                                 "out_w %d, %d parameters" % (len(hp.dilations), args.batch, T, tr.output_width, tr.n_params)},
                      "losses": losses}))
if world > 1:
    dist.destroy_process_group()
