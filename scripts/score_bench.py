#!/usr/bin/env python
"""WaveNet scoring beside the training step, BASELINE configs[1]'s model (30 layers, hop 300, MoL, S = 512).  One leg per process, so
that the processes of two builds can alternate on one box (`--root` names a checkout with its own library, e.g. the parent commit):
    --leg train    twv_wavenet_train_loss_grad and the whole WaveNetTrainer.step (the `train` leg of bench.py) on one 64 x 7800 batch
    --leg score    twv_wavenet_score_windows on the same 64 x 7800 batch (64 slots, one 7800-sample window each)
    --leg ragged   WaveNetScorer.score on 64 utterances of RandomState(0).randint(80, 641) frames (the list of scripts/queue_bench.py)
                   at --slots with the default window: scored samples per second (host staging included) and the share of rows that
                   are halo rows computed a second time
    --leg torch    the PyTorch-ROCm float32 composition of the same forward on the same batch (tests/torch_train_ref.py: upsample,
                   network_mm, mol_loss, under no_grad)
--width W (32, 64, 128) sets residual_channels = dilation_channels of the score and torch legs (the training step is built for 32).
`--summarise_wide` turns the log's score / torch legs at the three widths, and the rocprofv3 kernel statistics of one score leg per
width under --stats_dir/w<W>/ (rocprofv3 --kernel-trace --stats ... -- python scripts/score_bench.py --leg score --width W), into
--out (default profiles/wavenet_score_wide_bench.txt).
Each leg appends one JSON line to --log; `--summarise` turns the log into --out (default profiles/wavenet_score_bench.txt).
Times are medians of --reps launches, each between two device synchronisations."""
import argparse, json, os, sys, time
ap = argparse.ArgumentParser()
ap.add_argument("--leg", choices=("train", "score", "ragged", "torch")); ap.add_argument("--width", type=int, default=32)
ap.add_argument("--summarise_wide", action="store_true"); ap.add_argument("--stats_dir", default=None)
ap.add_argument("--root", default=None); ap.add_argument("--label", default="")
ap.add_argument("--slots", type=int, default=8); ap.add_argument("--reps", type=int, default=7); ap.add_argument("--summarise", action="store_true")
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap.add_argument("--log", default=os.path.join(HERE, "build", "score_bench", "legs.jsonl"))
ap.add_argument("--out", default=None)
args = ap.parse_args()
args.out = args.out or os.path.join(HERE, "profiles", "wavenet_score_wide_bench.txt" if args.summarise_wide else "wavenet_score_bench.txt")
PEAK_F32_MFMA = 157.3e12                                     # FLOP/s, MI355X: 256 CUs x 4 SIMDs x 64 FLOP/clk x 2.4 GHz


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


if args.summarise_wide:
    import csv, glob
    rows = [json.loads(l) for l in open(args.log)]
    out = ["WaveNet scoring at residual = dilation width 32, 64 and 128 (scripts/score_bench.py --summarise_wide): one 64 x 7800 batch of the",
           "30-layer model (hop 300, MoL, S = 512), forward only; medians of the repeats inside a process, processes alternating on one box", ""]
    for W in (32, 64, 128):
        sc = [r for r in rows if r["leg"] == "score" and r.get("width", 32) == W and r["build"] == "this"]
        to = [r for r in rows if r["leg"] == "torch" and r.get("width", 32) == W]
        if not sc:
            continue
        v = [r["score_ms"] for r in sc]
        out.append("width %3d  twv_wavenet_score_windows          %s  median %.3f ms  (workspace %.0f MB, mean nll %.6f)" % (
            W, " ".join("%.3f" % x for x in v), median(v), sc[0]["workspace_mb"], sc[0]["mean_nll"]))
        if to:
            t = [r["torch_ms"] for r in to]
            out.append("width %3d  PyTorch float32 composition        %s  median %.3f ms  (mean nll %.6f) -> own kernels %.2f x the composition's time" % (
                W, " ".join("%.3f" % x for x in t), median(t), to[0]["mean_nll"], median(v) / median(t)))
        f = sorted(glob.glob(os.path.join(args.stats_dir or "", "w%d" % W, "**", "*kernel_stats.csv"), recursive=True))
        if f:
            ks = list(csv.DictReader(open(f[-1])))
            lay = [r for r in ks if "sc_layer" in r["Name"]]
            passes = sum(int(r["Calls"]) for r in lay) / 30.0
            lay_ms = sum(float(r["TotalDurationNs"]) for r in lay) / passes / 1e6
            all_ms = sum(float(r["TotalDurationNs"]) for r in ks if "fillBuffer" not in r["Name"]) / passes / 1e6
            fl = sc[0]["layer_mfma_flops"]
            out.append("width %3d  layer kernels (%s): %.3f ms of %.3f ms kernel time per pass (%.1f %%); %.2f TFLOP executed on the matrix cores -> %.1f TFLOP/s = %.1f %% of the %.1f TFLOP/s f32-MFMA peak" % (
                W, lay[0]["Name"].split("(")[0].replace("void ", ""), lay_ms, all_ms, 100 * lay_ms / all_ms, fl / 1e12, fl / lay_ms / 1e9, 100 * fl / (lay_ms * 1e-3) / PEAK_F32_MFMA, PEAK_F32_MFMA / 1e12))
        out.append("")
    for leg, key, what in (("score", "score_ms", "width 32 scoring"), ("train", "step_ms", "WaveNetTrainer.step"), ("train", "loss_grad_ms", "twv_wavenet_train_loss_grad")):
        ab = {}
        for build in ("parent", "this"):
            ab[build] = [r[key] for r in rows if r["leg"] == leg and r["build"] == build and r.get("width", 32) == 32]
        if ab["parent"] and ab["this"]:
            a, b = ab["parent"], ab["this"]
            out.append("%-28s parent %s (median %.3f ms, spread %.2f %%)   this %s (median %.3f ms): %+.2f %%" % (
                what, " ".join("%.3f" % x for x in a), median(a), 100 * (max(a) - min(a)) / median(a), " ".join("%.3f" % x for x in b), median(b), 100 * (median(b) / median(a) - 1)))
    open(args.out, "w").write("\n".join(out) + "\n")
    print("\n".join(out))
    sys.exit(0)

if args.summarise:
    rows = [json.loads(l) for l in open(args.log)]
    out = ["WaveNet scoring beside the training step (scripts/score_bench.py): 30 layers, hop 300, MoL, S = 512; medians of the repeats inside",
           "a process, processes of the two builds alternating on one box", ""]
    for leg, key, what in (("train", "loss_grad_ms", "twv_wavenet_train_loss_grad, 64 x 7800"), ("train", "step_ms", "WaveNetTrainer.step, 64 x 7800 (bench.py's train leg)"),
                           ("score", "score_ms", "twv_wavenet_score_windows, 64 x 7800")):
        for build in sorted({r["build"] for r in rows if r["leg"] == leg}):
            v = [r[key] for r in rows if r["leg"] == leg and r["build"] == build and r.get("width", 32) == 32]
            out.append("%-58s %-8s %s  median %.3f ms  spread %.2f %%" % (what, build, " ".join("%.3f" % x for x in v), median(v), 100 * (max(v) - min(v)) / median(v)))
    t = [r["loss_grad_ms"] for r in rows if r["leg"] == "train" and r["build"] == "parent"]
    s = [r["score_ms"] for r in rows if r["leg"] == "score" and r.get("width", 32) == 32]
    if t and s:
        out += ["", "(a) forward-only scoring of the batch takes %.3f of the parent's loss + gradient pass (%.3f ms against %.3f ms)" % (median(s) / median(t), median(s), median(t))]
    a = [r["step_ms"] for r in rows if r["leg"] == "train" and r["build"] == "parent"]
    b = [r["step_ms"] for r in rows if r["leg"] == "train" and r["build"] == "this"]
    if a and b:
        out += ["(c) training step: this build %.3f ms against the parent's %.3f ms (%+.2f %%); the parent's own spread %.2f %%"
                % (median(b), median(a), 100 * (median(b) / median(a) - 1), 100 * (max(a) - min(a)) / median(a))]
    out += ["", "(b) 64 utterances of 89 .. 640 frames, default window:"]
    for r in rows:
        if r["leg"] == "ragged":
            out.append("    slots %2d window %d: %d windows in %d batches, %d scored samples in %s s -> median %.0f samples/s; halo rows recomputed: %.1f %% of the rows"
                       % (r["slots"], r["window"], r["windows"], r["batches"], r["scored"], " ".join("%.3f" % x for x in r["seconds"]), r["scored"] / median(r["seconds"]), 100 * r["halo_share"]))
    open(args.out, "w").write("\n".join(out) + "\n")
    print("\n".join(out))
    sys.exit(0)

ROOT = os.path.abspath(args.root) if args.root else HERE
sys.path.insert(0, ROOT)
import ctypes as C
import numpy as np, torch
import twvk_amd
from twvk_amd import _lib
from twvk_amd.wavenet import WaveNetModel, _ptr, _stream
assert torch.cuda.is_available(), "a measurement needs the GPU"
hp = twvk_amd.default_hparams()
dil = [2 ** i for i in range(10)] * 3


def model(batch, width=32):
    return WaveNetModel(batch, dil, hp.filter_width, width, width, 512, quantization_channels=256, out_channels=30, use_biases=True, scalar_input=True,
                        initial_filter_width=32, global_condition_channels=32, global_condition_cardinality=2, local_condition_channels=80,
                        upsample_factor=[5, 5, 12], train_mode=True, device="cuda:0")


def timed(fn, reps):
    fn(); fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(); out.append((time.perf_counter() - t0) * 1e3)
    return out


rec = {"leg": args.leg, "build": "parent" if args.root else "this", "label": args.label, "library": _lib.lib().twv_version().decode(), "width": args.width}
rng = np.random.RandomState(100)
B, T = 64, 7800
audio = (rng.rand(B, T) - 0.5).astype(np.float32)
lc = (rng.randn(B, T // 300, 80) * 0.5).astype(np.float32)
gc = rng.randint(0, 2, B).astype(np.int32)
if args.leg == "train":
    from twvk_amd.train import WaveNetTrainer
    tr = WaveNetTrainer(model(B), hp, sample_size=8000)
    tr.init_weights(seed=0)
    a, l, g = torch.from_numpy(audio).cuda(), torch.from_numpy(lc).cuda(), torch.from_numpy(gc).cuda()
    rec["loss_grad_ms"] = median(timed(lambda: tr.loss_and_gradients(a, l, g), args.reps))
    rec["step_ms"] = median(timed(lambda: tr.step(a, l, g), args.reps))
elif args.leg == "score":
    from twvk_amd.score import WaveNetScorer
    from twvk_amd import weights as W
    sc = WaveNetScorer(model(B, args.width) if args.width != 32 else model(B), window=T, slots=B)
    sc.load_weights(W.random_tensors(sc.net.specs, seed=0, scale=0.05))
    # MFMA FLOPs the layer kernels execute: per 32-row tile W / 32 channel blocks of 2 W (two taps, filter and gate) + 16 W / 32 (dense)
    # v_mfma_f32_32x32x2_f32 of 4096 FLOP each; a layer walks the tiles from its receptive offset on
    nb, off, rec["layer_mfma_flops"] = args.width // 32, 31, 0
    for d_ in dil:
        off += d_
        rec["layer_mfma_flops"] += B * ((T - 1 + 31) // 32 - off // 32) * nb * (2 * args.width + 16 * nb) * 4096
    a, l, g = torch.from_numpy(audio).cuda(), torch.from_numpy(lc).cuda(), torch.from_numpy(gc).cuda()
    ws = torch.empty(sc._L.twv_wavenet_score_workspace_bytes(sc._h) // 4, dtype=torch.float32, device="cuda")
    nll = torch.empty((B, sc.width), dtype=torch.float32, device="cuda")
    lens = np.full(B, T, np.int32)
    rec["score_ms"] = median(timed(lambda: _lib.check(sc._L.twv_wavenet_score_windows(sc._h, _ptr(sc.params), _ptr(a), _ptr(l), _ptr(g), lens.ctypes.data_as(C.c_void_p),
                                                                                   _ptr(ws), _ptr(nll), _stream())), args.reps))
    rec["workspace_mb"] = ws.numel() * 4 / 1e6
    rec["mean_nll"] = float(nll.double().mean().item())
elif args.leg == "torch":
    sys.path.insert(0, os.path.join(HERE, "tests"))
    import torch_train_ref as R
    from twvk_amd import weights as W
    net = model(B, args.width) if args.width != 32 else model(B)
    P = {k: torch.from_numpy(v).cuda() for k, v in W.random_tensors(net.specs, seed=0, scale=0.05).items()}
    cfg = dict(dilations=dil, initial_filter_width=32, use_biases=True, upsample_factor=(5, 5, 12))
    a, l, g = torch.from_numpy(audio).cuda(), torch.from_numpy(lc).cuda(), torch.from_numpy(gc).cuda()
    rf = R.receptive_field(cfg)
    keep = {}

    def forward():
        with torch.no_grad():
            U = R.upsample(l, [P["wavenet/upsample%d/kernel" % i] for i in range(3)], cfg["upsample_factor"])
            keep["nll"] = R.mol_loss(R.network_mm(P, cfg, a[:, None, :-1], U, g), a[:, rf:, None])
    rec["torch_ms"] = median(timed(forward, args.reps))
    rec["mean_nll"] = float(keep["nll"].double().mean().item())
else:
    from twvk_amd.score import WaveNetScorer, plan
    from twvk_amd import weights as W
    frames = np.random.RandomState(0).randint(80, 641, size=64).tolist()
    sc = WaveNetScorer(model(args.slots), slots=args.slots)
    sc.load_weights(W.random_tensors(sc.net.specs, seed=0, scale=0.05))
    audios = [(rng.rand(f * 300) - 0.5).astype(np.float32) for f in frames]
    mels = [(rng.randn(f, 80) * 0.5).astype(np.float32) for f in frames]
    gcs = (np.arange(64) % 2).tolist()
    p = plan([len(a) for a in audios], sc.window, sc.rf, sc.hop, sc.slots)
    rows = p.table.reshape(-1, 5); rows = rows[rows[:, 0] >= 0]
    computed = int(rows[:, 2].sum())
    sc.score(audios[:2], mels[:2], gcs[:2]); torch.cuda.synchronize()
    secs = []
    for _ in range(3):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        out = sc.score(audios, mels, gcs)
        torch.cuda.synchronize(); secs.append(time.perf_counter() - t0)
    rec.update(slots=args.slots, window=sc.window, windows=p.n_windows, batches=len(p.table), scored=int(sum(v.numel() for v in out)), seconds=secs,
               halo_share=(computed - sum(len(a) for a in audios)) / computed, frames=[min(frames), max(frames)])
os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
with open(args.log, "a") as fh:
    fh.write(json.dumps(rec) + "\n")
print(json.dumps(rec))
