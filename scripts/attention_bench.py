#!/usr/bin/env python
"""Tacotron pass time per attention type at the bench geometry (B = 32 utterances of 100 tokens + EOS, 200 decoder steps, post-CBHG and
linear on): the default bah_mon_norm on the library's own kernel choice (the XCD-resident decoder), bah_mon_norm forced onto the split
decoder (decoder_groups 8), and the other types (split decoder only).  One JSON line per case."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import twvk_amd
from twvk_amd.tacotron import Tacotron
from torch_attention_ref import random_tensors

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--steps", type=int, default=5, help="timed passes per case (the median is reported)")
ap.add_argument("--types", default="bah_mon_norm,bah_mon_norm@8,bah,loc_sen",
                help="comma-separated attention types; '@G' forces decoder_groups G")
args = ap.parse_args()
N, T = args.batch, 101
rng = np.random.RandomState(1)
tok = rng.randint(2, 80, (N, T)).astype(np.int32); tok[:, -1] = 1
ln = np.full(N, T, np.int32); spk = (np.arange(N) % 2).astype(np.int32)
for case in args.types.split(","):
    at, _, groups = case.partition("@")
    hp = twvk_amd.default_hparams()
    hp.attention_type = at
    m = Tacotron(hp, num_speakers=2)
    m.load_weights(random_tensors(m.specs, 0))
    if groups:
        m.set_option("decoder_groups", int(groups))
    m.infer(tok, ln, spk); torch.cuda.synchronize()
    times = []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        mel, lin, al = m.infer(tok, ln, spk)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    dt = float(np.median(times))
    print(json.dumps({"attention_type": at, "decoder_groups": int(groups) if groups else 0, "kernel": m.decoder_kernel_name(N, T),
                      "ms_per_pass": dt * 1e3, "ms_min": min(times) * 1e3, "mel_frames_per_s": N * hp.max_iters * hp.reduction_factor / dt,
                      "finite": bool(torch.isfinite(mel).all().item())}), flush=True)
    del m
