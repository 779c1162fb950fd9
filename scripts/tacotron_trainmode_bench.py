#!/usr/bin/env python
"""Times of one Tacotron training-mode step (TacotronTrainer(training=True).step) at the default geometry -- B = 8 and
B = 32, 101 tokens, 200 decoder steps (T_out = 1000 frames), the weights of scripts/tacotron_bench.py -- by phase from events on its stream
(forward_targets + masks + the three recording forwards + add_loss; the three backwards with their range copies; the speaker side;
gradient conversion + clip + Adam + moving update + refold + re-pack + the read-back of the batch norm tensors) and from the host, beside
the evaluation-graph step (training=False) of the same build in the same process.  Medians of --passes steps.  Writes --out (default
profiles/tacotron_trainmode_bench.txt).  Needs the GPU."""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np, torch
import twvk_amd
from twvk_amd import _lib
from twvk_amd.tacotron import Tacotron
from tacotron_targets_bench import random_tensors
from tacotron_train_bench import STEPS, T, TimedTrainer


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tacotron_trainmode_bench.txt"))
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--batches", default="8,32")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    hp = twvk_amd.default_hparams()
    lines = ["One Tacotron training step, training mode (batch-statistics batch norm, dropout, moving averages) beside the evaluation graph, default",
             "geometry: 101 tokens, 200 decoder steps (T_out 1000), every length 101, two speakers (scripts/tacotron_trainmode_bench.py; medians of %d steps, ms)" % args.passes,
             "library %s on %s, torch %s" % (_lib.lib().twv_version().decode(), torch.cuda.get_device_name(0), torch.__version__), "",
             "%-22s %14s %14s %12s %16s %10s" % ("", "forwards+loss", "backwards", "speaker", "update+refold", "host")]
    for N in [int(b) for b in args.batches.split(",")]:
        rng = np.random.RandomState(1)
        tok = rng.randint(2, 80, (N, T)).astype(np.int32); tok[:, -1] = 1
        ln = np.full(N, T, np.int32); spk = (np.arange(N) % 2).astype(np.int32)
        TO = STEPS * hp.reduction_factor
        tg = torch.from_numpy(rng.uniform(-4, 4, (N, TO, hp.num_mels)).astype(np.float32)).cuda()
        lt = torch.from_numpy(rng.uniform(-4, 4, (N, TO, hp.num_freq)).astype(np.float32)).cuda()
        for training in (False, True):
            m = Tacotron(hp, num_speakers=2)
            m.load_weights(random_tensors(m.specs))
            tr = TimedTrainer(m, training=training, seed=1)
            walls, phases = [], []
            for i in range(args.passes + 1):
                torch.cuda.synchronize(); t0 = time.perf_counter()
                loss = tr.step(tok, ln, spk, tg, lt)["loss"]
                torch.cuda.synchronize(); walls.append((time.perf_counter() - t0) * 1e3)
                phases.append(tr.phases())
                assert np.isfinite(loss), loss
            ph = np.median(np.asarray(phases[1:]), axis=0)
            lines.append("%-22s %14.2f %14.2f %12.3f %16.2f %10.1f" % ("B = %d %s" % (N, "training" if training else "evaluation"), ph[0], ph[1], ph[2], ph[3],
                                                                     float(np.median(walls[1:]))))
            del tr, m
    lines += ["", "(evaluation: forward_targets + add_loss, then each pass's forward and backward in one call; training: every recording forward in the first column)"]
    text = "\n".join(lines) + "\n"
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
