#!/usr/bin/env python
"""Seconds per step of the Tacotron training loop over the same 64 feeder batches of varying shape, at the reference's batch
32 and the default hparams, training mode, two speakers; synthetic examples (seeded, 150 .. 995 frames, 30 .. 100 tokens) written to a
temporary directory and read by DataFeederTacotron.  The batches' examples are loaded once and held in memory, so no route pays for the disk.

Routes, one trainer each, alternating over --rounds rounds in one process (host clock around steps that end in a device synchronise):
  new            pack -> one copy -> twv_tacotron_batch_stage one batch ahead on the feed stream (thread), reshaped handles, reserved workspaces
  new-noprefetch the same with the staging in line
  churn          staged device tensors, but _drop_grad_handles() before each step: handles created at every shape
  parent         prepare_batch on the host (padding), numpy arrays into step(), _drop_grad_handles() before each step: the step as it was
  floor          step() a second time on each batch's device tensors with warm handles at that shape: what a feed costing nothing would
                 reach; it takes its turn in every round
Reported: each route's mean and median, handle churn per step (churn - new-noprefetch), host padding + upload per step (parent - churn),
the staging kernels' time from device events with their bytes (packed words read + outputs written) per second beside the measured HBM
copy rate of 6.29 TB/s (8.0 TB/s spec), on cold buffers (three sets in turn) and, marked as cache-assisted, on warm ones.  `--bench FILE ...`:
files with bench.py's JSON line of this build and of the parent build, alternating (this, parent, this, ...) as they were run in one visit;
their headlines are printed last.  Writes --out (default profiles/tacotron_train_loop_bench.txt).  Needs the GPU."""
import argparse, json, os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import twvk_amd
from twvk_amd import _lib
from twvk_amd.tacotron import Tacotron
from twvk_amd.tacotron_feed import BATCH_KEYS, BatchStager, DataFeederTacotron, ROW_DTYPE, ROW_WORDS, pack_batch, prepare_batch, stage_packed, staged_batches, target_frames
from twvk_amd.tacotron_train import TacotronTrainer

HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12


def write_examples(root, hp, per_speaker, seed):
    rng = np.random.RandomState(seed)
    dirs = []
    for s in range(2):
        d = os.path.join(root, "speaker_%d" % s)
        os.makedirs(d)
        dirs.append(d)
        for i in range(per_speaker):
            n_frames, n_tokens = int(rng.randint(150, 996)), int(rng.randint(30, 101))
            np.savez(os.path.join(d, "%04d.npz" % i), tokens=rng.randint(1, 80, n_tokens).astype(np.int32),
                     mel=rng.uniform(-4, 4, (n_frames, hp.num_mels)).astype(np.float32), linear=rng.uniform(-4, 4, (n_frames, hp.num_freq)).astype(np.float32))
    return dirs


class ListFeeder(object):
    """the recorded batches again, in order (what staged_batches reads of a feeder)"""

    def __init__(self, hp, batches):
        self._hp, self._batches, self._k = hp, batches, 0

    def next_examples(self):
        b = self._batches[self._k % len(self._batches)]
        self._k += 1
        return list(b)


def args_of(batch):
    return (batch["inputs"], batch["input_lengths"], batch["speaker_id"], batch["mel_targets"], batch["linear_targets"], batch["loss_coeff"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=64)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--per-speaker", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tacotron_train_loop_bench.txt"))
    ap.add_argument("--bench", nargs="+", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    hp = twvk_amd.default_hparams()
    r = hp.reduction_factor
    with tempfile.TemporaryDirectory() as tmp:
        dirs = write_examples(tmp, hp, a.per_speaker, 0)
        feeder = DataFeederTacotron(dirs, hp, a.batch, 8, "train", random_seed=123)
        cache, batches = {}, []
        for _ in range(a.batches):
            batches.append([cache.setdefault((ex["speaker_id"], ex["name"]), ex) for ex in feeder.next_examples()])
    shapes = [(max(len(ex["tokens"]) for ex in b), target_frames(b, r)) for b in batches]

    def trainer():
        m = Tacotron(hp, num_speakers=2)
        t = TacotronTrainer(m, training=True, seed=1)
        t.init_weights(0)
        return t
    names = ("new", "new-noprefetch", "churn", "parent")
    T = {n: trainer() for n in names}
    for n in ("new", "new-noprefetch"):
        T[n].model.reserve_gradients(a.batch, max(s[0] for s in shapes), max(s[1] for s in shapes) // r)
    stagers = {n: BatchStager("cuda:0", hp.num_mels, hp.num_freq) for n in ("new", "new-noprefetch", "churn")}
    sync = torch.cuda.synchronize

    def run(name, count):
        t, times = T[name], []
        if name == "parent":
            for b in batches[:count]:
                t0 = time.perf_counter()
                host = prepare_batch(list(b), r)
                t.model._drop_grad_handles()
                t.step(*args_of(host))
                sync()
                times.append(time.perf_counter() - t0)
            return times
        it = staged_batches(ListFeeder(hp, batches), stagers[name], count=count, prefetch=(name == "new"))
        t0 = time.perf_counter()
        for _, batch in it:
            if name == "churn":
                t.model._drop_grad_handles()
            t.step(*args_of(batch))
            sync()
            t1 = time.perf_counter()
            times.append(t1 - t0)
            t0 = t1
        return times
    def run_floor():
        """warm handles at each batch's own shape: the second of two steps on the same device tensors"""
        t, st, times = T["new-noprefetch"], stagers["new-noprefetch"], []
        for b in batches:
            batch = st.stage(list(b), r)
            t.step(*args_of(batch)); sync()
            t0 = time.perf_counter()
            t.step(*args_of(batch)); sync()
            times.append(time.perf_counter() - t0)
        return times
    for n in names:                                                # every route once over a few batches: code objects, rocBLAS, pinned memory
        run(n, 4)
    res = {n: [] for n in names + ("floor",)}
    for _ in range(a.rounds):                                      # the floor takes its turn in every round, as the routes do
        for n in names:
            res[n].append(run(n, a.batches))
        res["floor"].append(run_floor())
    # the staging launches alone, device events on the stream that runs them.  warm: the same buffers again straight after a run on them
    # (a batch's source and outputs, 167 MB at the largest, fit the 256 MB Infinity Cache: NOT an HBM figure).  cold: three sets of
    # buffers in turn, three times round, so that two other sets (twice the batch's bytes, more than the cache for most batches) have
    # passed through since a set was last touched
    def timed(dev, table, lay, t_in, t_out, out):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        stage_packed(dev, table, lay, t_in, t_out, hp.num_mels, hp.num_freq, out=out)
        e1.record(); sync()
        return e0.elapsed_time(e1)
    warm_ms, cold_ms, stage_bytes = [], [], []
    for b, (t_in, t_out) in zip(batches, shapes):
        buf, lay = pack_batch(list(b), hp.num_mels, hp.num_freq)
        table = buf[lay["table_at"]:lay["table_at"] + ROW_WORDS * len(b)].view(ROW_DTYPE).copy()
        devs = [torch.from_numpy(buf.view(np.int32)).to("cuda:0") for _ in range(3)]
        outs = [stage_packed(d, table, lay, t_in, t_out, hp.num_mels, hp.num_freq) for d in devs]      # (every set written once)
        sync()
        cold_ms.append([timed(devs[k], table, lay, t_in, t_out, outs[k]) for _ in range(3) for k in range(3)])
        warm_ms.append([timed(devs[0], table, lay, t_in, t_out, outs[0]) for _ in range(3)])
        stage_bytes.append(4 * (lay["table_at"] + sum(outs[0][k].numel() for k in BATCH_KEYS)))
        del devs, outs
    L = _lib.lib()
    lines = ["The Tacotron training loop over the same %d feeder batches of varying shape, batch %d, default hparams, training mode, two speakers"
             % (a.batches, a.batch),
             "(scripts/tacotron_train_loop_bench.py; seconds per step by the host clock around steps that end in a device synchronise; %d rounds," % a.rounds,
             "routes alternating in one process; the examples are held in memory)",
             "library %s on %s, torch %s" % (L.twv_version().decode(), torch.cuda.get_device_name(0), torch.__version__),
             "shapes (T_in, T_out): T_in %d .. %d, T_out %d .. %d, %d different" % (min(s[0] for s in shapes), max(s[0] for s in shapes),
                                                                                   min(s[1] for s in shapes), max(s[1] for s in shapes), len(set(shapes))),
             "", "%-16s %s" % ("route", "  ".join("round %d mean / median" % (k + 1) for k in range(a.rounds)))]
    mean = {}
    for n in names + ("floor",):
        lines.append("%-16s %s" % (n, "  ".join("%9.4f / %9.4f   " % (np.mean(x), np.median(x)) for x in res[n])))
        mean[n] = float(np.mean([np.mean(x) for x in res[n]]))
    floor = float(np.mean([np.mean(x) for x in res["floor"]]))
    spread = max(abs(np.mean(res[n][0]) - np.mean(res[n][-1])) for n in res)
    sb = np.asarray(stage_bytes, np.float64)
    cold, warm = np.median(np.asarray(cold_ms), axis=1) * 1e-3, np.median(np.asarray(warm_ms), axis=1) * 1e-3
    rate_c, rate_w = float(sb.sum() / cold.sum()), float(sb.sum() / warm.sum())
    lines += ["(floor: the second of two steps on each batch's device tensors, warm handles at that shape)",
              "largest difference between a route's rounds: %.4f s -- differences below it are not measured" % spread, "",
              "handle churn per step (churn - new-noprefetch)        %9.4f s" % (mean["churn"] - mean["new-noprefetch"]),
              "host padding + upload per step (parent - churn)       %9.4f s" % (mean["parent"] - mean["churn"]),
              "new - floor %+.4f s, new-noprefetch - floor %+.4f s%s" % (mean["new"] - floor, mean["new-noprefetch"] - floor,
                                                                        " (new - floor is inside the spread between rounds)" if abs(mean["new"] - floor) <= spread else ""),
              "new route against the parent's route                  %9.4f s per step (%.1f %% of the parent's)" % (mean["new"] - mean["parent"],
                                                                                                                 100.0 * mean["new"] / mean["parent"]),
              "staging (three launches a batch, device events, median of the repeats per batch, %.1f MB a batch = packed words read + outputs written):" % (sb.mean() / 1e6),
              "  cold (three buffer sets in turn, 9 samples a batch): mean %.3f ms, %.2f TB/s = %.0f %% of the measured HBM copy rate (6.29 TB/s), %.0f %% of the 8.0 TB/s spec"
              % (1e3 * cold.mean(), rate_c / 1e12, 100 * rate_c / HBM_MEASURED, 100 * rate_c / HBM_SPEC),
              "  warm (the same buffers again, 3 samples a batch; a batch fits the 256 MB Infinity Cache, so this is cache-assisted, not an HBM figure): mean %.3f ms, %.2f TB/s"
              % (1e3 * warm.mean(), rate_w / 1e12)]
    if mean["new"] >= mean["parent"]:
        lines.append("the new route is NOT faster than the parent's route here")
    if a.bench:
        lines += ["", "bench.py --gpus 1 --steps 2 --warmup 1, this build and the parent build alternating in one visit (samples/s; ms per step):"]
        for k, path in enumerate(a.bench):
            line = [json.loads(l) for l in open(path) if l.startswith("{")][-1]
            lines.append("  %-13s %9.0f  (%.2f)" % ("this build" if k % 2 == 0 else "parent build", line["value"], line["ms_per_step"]))
    text = "\n".join(lines) + "\n"
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
