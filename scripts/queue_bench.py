#!/usr/bin/env python
"""Delivered samples/s of a list of utterances of unequal lengths: padded batches through `generate` against the utterance queue
(`generate_list`) at several chunk sizes and both orders.  BASELINE configs[1]'s model (30 layers, hop 300, MoL) on 8 slots, 64
utterances of RandomState(0).randint(80, 641) frames.  The variants run in alternation, `--reps` times; wall time is a host clock
around calls that end in a device synchronise (status()).  Writes the table to --out (default profiles/utterance_queue_bench.txt)."""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
from helpers import make_model, mol_uniforms
import twvk_amd  # noqa: F401
from twvk_amd import queue as Q, weights as W

ap = argparse.ArgumentParser()
ap.add_argument("--slots", type=int, default=8); ap.add_argument("--utterances", type=int, default=64)
ap.add_argument("--min-frames", type=int, default=80); ap.add_argument("--max-frames", type=int, default=640)
ap.add_argument("--chunks", default="1,2,4,8,16,32"); ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--big-slots", type=int, default=32, help="one more generate_list run at this many slots (0: none)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "utterance_queue_bench.txt"))
args = ap.parse_args()
assert torch.cuda.is_available(), "a measurement needs the GPU"
HOP, NR = 300, 10
B, n = args.slots, args.utterances
lengths = np.random.RandomState(0).randint(args.min_frames, args.max_frames + 1, size=n).tolist()
chunks = [int(c) for c in args.chunks.split(",")]
dil = [2 ** i for i in range(10)] * 3
specs = W.tensor_specs(len(dil), 32, 32, 512, 256, 30, True, 32, True, 32, 2, 80, (5, 5, 12))
tensors = W.random_tensors(specs, seed=0, scale=0.05)
m = make_model(B, dil, tensors)
rng = np.random.RandomState(1)
mels = [torch.from_numpy(rng.uniform(-4, 4, (t, 80)).astype(np.float32)).cuda() for t in lengths]
us = [torch.from_numpy(mol_uniforms(1, t * HOP, NR, seed=2 + i)[0]).cuda() for i, t in enumerate(lengths)]
gc = (np.arange(n) % 2).astype(np.int32)
seeds = (2 * rng.rand(n) - 1).astype(np.float32)
delivered = sum(lengths) * HOP


def padded():
    """FIFO batches of B through generate, each at its batch's longest length; (seconds, steps, [(steps, seconds) per batch])"""
    t0 = time.perf_counter(); steps = 0; per = []
    outs = []
    for p in range(0, n, B):
        idx = list(range(p, min(p + B, n)))
        tmax = max(lengths[i] for i in idx)
        mel = torch.zeros((B, tmax, 80), dtype=torch.float32, device="cuda")
        u = torch.full((B, tmax * HOP, NR + 1), 0.5, dtype=torch.float32, device="cuda")
        g = np.zeros(B, np.int32); s = np.zeros(B, np.float32)
        for j, i in enumerate(idx):
            mel[j, :lengths[i]] = mels[i]; u[j, :lengths[i] * HOP] = us[i]; g[j] = gc[i]; s[j] = seeds[i]
        m.queue_initializer()
        torch.cuda.synchronize(); b0 = time.perf_counter()
        out = m.generate(m.create_upsample(mel), g, s, u, check=False)
        m.status()
        per.append((tmax * HOP, time.perf_counter() - b0))
        outs += [out[j, :lengths[i] * HOP].clone() for j, i in enumerate(idx)]
        steps += tmax * HOP
    return time.perf_counter() - t0, steps, per, outs


def queued(model, k, order):
    t0 = time.perf_counter()
    outs = model.generate_list(mels, gc, seeds, us, chunk_frames=k, order=order, check=False)      # ends in status()
    return time.perf_counter() - t0, outs


variants = [("padded", None, None)] + [("queue", k, o) for k in chunks for o in Q.ORDERS]
times = {v: [] for v in variants}
step_us = []
ref = None
# warm-up: every launch shape the timed window uses (code objects, allocator), on the first frames of 2 * B utterances
wf = min(40, min(lengths))
wm, wu = [x[:wf] for x in mels[:2 * B]], [x[:wf * HOP] for x in us[:2 * B]]
m.queue_initializer()
m.generate(m.create_upsample(torch.stack(wm[:B])), gc[:B], seeds[:B], torch.stack(wu[:B]))
for k in chunks:
    m.generate_list(wm, gc[:2 * B], seeds[:2 * B], wu, chunk_frames=k, check=False)
for r in range(args.reps):
    for v in variants:                                   # in alternation: one pass over all variants per repetition
        if v[0] == "padded":
            t, psteps, per, outs = padded()
            step_us += [1e6 * s / st for st, s in per]
            if ref is None:
                ref = outs
        else:
            t, outs = queued(m, v[1], v[2])
            assert all(torch.equal(a, b) for a, b in zip(outs, ref)), "the queue's samples differ from the padded batches'"
        times[v].append(t)
unchunked = float(np.median(step_us))
lines = ["utterance queue bench: %s, %d slots, %d utterances of %d..%d frames (RandomState(0)), %d delivered samples, %d repetitions in alternation"
         % (m.kernel_name(), B, n, min(lengths), max(lengths), delivered, args.reps),
         "step time of an unchunked launch (median over the padded batches of this run): %.3f us" % unchunked,
         "samples of every queue variant compared with the padded batches': bit-identical",
         "",
         "%-26s %8s %14s %10s %10s %10s %16s %12s %14s" % ("variant", "chunks", "makespan_steps", "wall_s", "min_s", "max_s", "delivered_samp/s", "vs_padded", "us_per_chunk")]
pad_t = float(np.median(times[variants[0]]))
assert psteps == Q.padded_makespan_frames(lengths, B) * HOP
fit = []
for v in variants:
    t = float(np.median(times[v]))
    if v[0] == "padded":
        name, nch, steps, over = "padded fifo batches", (n + B - 1) // B, psteps, float("nan")
    else:
        pl = Q.plan(lengths, B, v[1], v[2])
        name, nch, steps = "queue k=%d %s" % (v[1], v[2]), pl.makespan, pl.makespan * v[1] * HOP
        over = 1e6 * (t - steps * unchunked * 1e-6) / nch
        fit.append((nch, t - steps * unchunked * 1e-6))
    lines.append("%-26s %8d %14d %10.3f %10.3f %10.3f %16.0f %12.3f %14.1f" % (name, nch, steps, t, min(times[v]), max(times[v]), delivered / t, pad_t / t, over))
if len(fit) > 1:
    slope, icpt = np.polyfit([f[0] for f in fit], [f[1] for f in fit], 1)
    lines.append("")
    lines.append("least-squares line through (chunks, wall_s - makespan_steps * unchunked step time) of the %d queue variants: %.1f us per chunk + %.1f ms per call"
                 % (len(fit), 1e6 * slope, 1e3 * icpt))
    lines.append("(us_per_chunk above divides the same difference by the chunk count alone, the per-call part included)")
lines.append("")
lines.append("analytic ratio padded / queue makespan (steps): " + ", ".join(
    "k=%d %s %.3f" % (k, o[:4], psteps / (Q.plan(lengths, B, k, o).makespan * k * HOP)) for k in chunks for o in Q.ORDERS))
if args.big_slots:
    big = make_model(args.big_slots, dil, tensors)
    k = big.DEFAULT_CHUNK_FRAMES
    big.generate_list(wm, gc[:2 * B], seeds[:2 * B], wu, chunk_frames=k, check=False)
    ts = [queued(big, k, "longest_first")[0] for _ in range(args.reps)]
    pl = Q.plan(lengths, args.big_slots, k, "longest_first")
    lines.append("")
    lines.append("%d slots, %s, k=%d longest_first: makespan %d steps in %d chunks, wall %.3f s (min %.3f, max %.3f), %.0f delivered samples/s, %.3f us per step of the makespan"
                 % (args.big_slots, big.kernel_name(), k, pl.makespan * k * HOP, pl.makespan, float(np.median(ts)), min(ts), max(ts), delivered / float(np.median(ts)),
                    1e6 * float(np.median(ts)) / (pl.makespan * k * HOP)))
txt = "\n".join(lines)
print(txt)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write(txt + "\n")
