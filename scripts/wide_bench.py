#!/usr/bin/env python
"""Times generation at residual / dilation widths 64 and 128 (wn_wide_generate_kernel) on the C2 stack (3 x [1..512], S = 512, MoL-30,
gc + lc) at batch 1, 8 and 64, and beside it the generic kernel (option xcd = 0) at width 32 for the same stack and batch.  Every timed
run sits behind a parity check of its first 600 steps against the CPU checker; a mismatch ends the script with status 1.
usage: python scripts/wide_bench.py [--steps 2400] [--batches 1,8,64] [--check 600] > profiles/wide_generation_bench.txt"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import twvk_amd
from twvk_amd import weights as W
from twvk_amd.wavenet import WaveNetModel

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=2400)
ap.add_argument("--batches", default="1,8,64")
ap.add_argument("--widths", default="32,64,128")
ap.add_argument("--check", type=int, default=600, help="steps compared with the CPU checker before timing")
args = ap.parse_args()
hp = twvk_amd.default_hparams()
dev = "cuda:0"
dil = [2 ** i for i in range(10)] * 3
T = args.steps // hp.hop_size * hp.hop_size
from oracle import oracle as O
O.build()

print("# C2 stack: %d layers, S = %d, MoL-%d, gc + lc, %d steps per run, device %s" % (len(dil), hp.skip_channels, hp.out_channels, T, torch.cuda.get_device_name(0)))
print("# %5s %5s %26s %12s %14s %10s" % ("width", "batch", "kernel", "us/step", "samples/s", "checked"))
ok = True
for width in [int(v) for v in args.widths.split(",")]:
    for B in [int(v) for v in args.batches.split(",")]:
        m = WaveNetModel(B, dil, hp.filter_width, width, width, hp.skip_channels, quantization_channels=hp.quantization_channels,
                         out_channels=hp.out_channels, use_biases=hp.use_biases, scalar_input=True, initial_filter_width=hp.initial_filter_width,
                         global_condition_channels=hp.gc_channels, global_condition_cardinality=2, local_condition_channels=hp.num_mels,
                         upsample_factor=hp.upsample_factor, train_mode=False, device=dev)
        if width == 32:
            m.set_option("xcd", 0)          # the yardstick: the generic kernel of the width-32 model
        tensors = W.random_tensors(m.specs, seed=0, scale=0.05)
        b2 = tensors["wavenet/conv1d_2/bias"].copy()
        b2[2 * (hp.out_channels // 3):] -= 5          # narrow mixture components: the samples stay off the +-1 clamp
        tensors["wavenet/conv1d_2/bias"] = b2
        m.load_weights(tensors)
        rq = np.random.RandomState(91)
        mel = rq.uniform(-4, 4, (B, T // hp.hop_size, hp.num_mels)).astype(np.float32)
        nu = hp.out_channels // 3 + 1
        lo, hi = np.float32(1e-5), np.float32(1.0 - 1e-5)
        u = (rq.random_sample((B, T, nu)).astype(np.float32) * (hi - lo) + lo).astype(np.float32)
        first = (2 * rq.rand(B) - 1).astype(np.float32)
        gc = (np.arange(B) % 2).astype(np.int32)
        Ud = m.create_upsample(torch.from_numpy(mel).to(dev))
        ud = torch.from_numpy(u).to(dev)
        n = min(args.check, T)
        nw = n if n else min(300, T)
        got = m.generate(Ud[:, :nw].contiguous(), gc, first, ud[:, :nw].contiguous()).cpu().numpy()    # also the warm-up
        exact = None
        if n:
            d = O.make_dims(dil, R=width, D=width)
            blob = O.blob_from_tensors(d, tensors)
            Uo = O.upsample(d, blob, mel[:, :(n + hp.hop_size - 1) // hp.hop_size])[:, :n].copy()
            O.set_threads(min(B, 16))
            want = O.generate_mol(d, blob, O.State(d, B), Uo, gc, first, u[:, :n])
            O.set_threads(1)
            exact = bool(np.array_equal(got, want)) and float(np.mean(np.abs(want) == 1.0)) <= 0.05
            ok = bool(ok and exact)
        m.queue_initializer()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.generate(Ud, gc, first, ud)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        res = {"width": width, "streams": B, "kernel": m.kernel_name(), "steps": T, "us_per_generation_step": dt / T * 1e6,
               "samples_per_s": B * T / dt, "checked_steps": n, "bit_exact": exact}
        print("  %5d %5d %26s %12.2f %14.0f %10s   %s" % (width, B, res["kernel"], res["us_per_generation_step"], res["samples_per_s"],
                                                          "exact" if exact else ("-" if exact is None else "MISMATCH"), json.dumps(res)))
        sys.stdout.flush()
        del m
sys.exit(0 if ok else 1)
