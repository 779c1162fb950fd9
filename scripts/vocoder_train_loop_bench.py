#!/usr/bin/env python
"""Seconds per step of the vocoder training loop over the same 64 feeder batches, at B = 8 (the hparams' wavenet_batch_size)
and B = 64 (the batch of scripts/train_bench.py), the 30-layer width-32 model and crops of 7800 samples.  A synthetic corpus is written
to a temporary directory with np.savez as preprocess.main writes it: two speakers, --per-speaker utterances each of 3 .. 8 s at 24 kHz with
the keys audio, mel and linear (+ time_steps, mel_frames) at the default hparams.

Routes, ONE trainer per batch size, taking turns over --rounds rounds in one process (host clock; every step ends in the loop's own
loss.item(), which drains the stream):
  parent         the loop as it stood: DataFeederWavenet, numpy arrays into step()
  host+prefetch  the same feeder behind wavenet_feed.PrefetchFeeder
  resident       wavenet_feed.DeviceFeederWavenet: the corpus in device memory, crops by twv_wavenet_crop_stage
  floor          step() on fixed device tensors with the same loss read: what a feed costing nothing would reach
Every run of a route starts its feeder anew with the same seeds, so all runs see the same 64 batches (checked on the first batch).
Reported per batch size: each route's mean and median per round, the largest difference between a route's rounds (differences below it
are not measured), parent - floor, resident - floor, whether resident <= parent outside that spread; the pack time and the packed bytes;
from device events, the time of next_batch() on the device (the copy of the picks + the crop launch) and of the launch alone.
`--step-log FILE`: the JSON lines `scripts/train_bench.py --log FILE` appended for this build and for the parent build (`--root`),
processes alternating; their ms per step are listed last: WaveNetTrainer.step alone beside the parent's.
Writes --out (default profiles/wavenet_train_loop_bench.txt).  Needs the GPU."""
import argparse, json, os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import twvk_amd
from twvk_amd import _lib
from twvk_amd.train import WaveNetTrainer
from twvk_amd.train_vocoder import DataFeederWavenet
from twvk_amd.wavenet import WaveNetModel
from twvk_amd.wavenet_feed import CorpusIndex, DeviceFeederWavenet, PrefetchFeeder, crop_stage

ROUTES = ("parent", "host+prefetch", "resident", "floor")


def write_corpus(root, hp, per_speaker, seed):
    rng = np.random.RandomState(seed)
    dirs = []
    for s in range(2):
        d = os.path.join(root, "speaker_%d" % s)
        os.makedirs(d)
        dirs.append(d)
        for i in range(per_speaker):
            frames = int(rng.randint(3 * hp.sample_rate // hp.hop_size, 8 * hp.sample_rate // hp.hop_size + 1))
            np.savez(os.path.join(d, "%04d.npz" % i), audio=rng.uniform(-0.5, 0.5, frames * hp.hop_size).astype(np.float32),
                     mel=rng.uniform(-4, 4, (frames, hp.num_mels)).astype(np.float32), linear=rng.uniform(-4, 4, (frames, hp.num_freq)).astype(np.float32),
                     time_steps=frames * hp.hop_size, mel_frames=frames)
    return dirs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=64)
    ap.add_argument("--sizes", default="8,64")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--per-speaker", type=int, default=100)
    ap.add_argument("--layers", type=int, default=30)
    ap.add_argument("--samples", type=int, default=8000)
    ap.add_argument("--step-log", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wavenet_train_loop_bench.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    hp = twvk_amd.default_hparams()
    hp.dilations = ([1, 2, 4, 8, 16, 32, 64, 128, 256, 512] * 8)[:a.layers]
    hp.sample_size = a.samples
    rf = WaveNetModel.calculate_receptive_field(hp.filter_width, hp.dilations, hp.scalar_input, hp.initial_filter_width)
    L = _lib.lib()
    lines = ["The vocoder training loop over the same %d feeder batches: %d layers, width %d, crops of %d samples, two speakers, %d utterances of 3 .. 8 s each"
             % (a.batches, a.layers, hp.residual_channels, a.samples // hp.hop_size * hp.hop_size, a.per_speaker),
             "(scripts/vocoder_train_loop_bench.py; seconds per step by the host clock, every step ends in loss.item(); %d rounds, routes taking turns in one process)" % a.rounds,
             "library %s on %s, torch %s" % (L.twv_version().decode(), torch.cuda.get_device_name(0), torch.__version__)]
    sync = torch.cuda.synchronize
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        dirs = write_corpus(tmp, hp, a.per_speaker, 0)
        lines.append("corpus written in %.1f s" % (time.perf_counter() - t0))
        for B in [int(x) for x in a.sizes.split(",")]:
            hp.wavenet_batch_size = B
            net = WaveNetModel(batch_size=B, dilations=hp.dilations, filter_width=hp.filter_width, residual_channels=hp.residual_channels,
                               dilation_channels=hp.dilation_channels, skip_channels=hp.skip_channels, quantization_channels=hp.quantization_channels,
                               out_channels=hp.out_channels, use_biases=hp.use_biases, scalar_input=hp.scalar_input,
                               initial_filter_width=hp.initial_filter_width, global_condition_channels=hp.gc_channels, global_condition_cardinality=2,
                               local_condition_channels=hp.num_mels, upsample_factor=hp.upsample_factor, train_mode=True, device="cuda:0")
            tr = WaveNetTrainer(net, hp)
            tr.init_weights(seed=0)
            t0 = time.perf_counter()
            index = CorpusIndex(dirs, B, rf, gc_enable=True, hp=hp)
            t_pack = time.perf_counter() - t0
            t0 = time.perf_counter()
            dev_feeder = DeviceFeederWavenet(index, "cuda:0")
            sync()
            t_upload = time.perf_counter() - t0
            np.random.seed(1234)
            fixed = tuple(t.clone() for t in dev_feeder.next_batch())
            first = {}

            def run(route, count):
                np.random.seed(1234)
                feeder = None
                if route == "parent":
                    feeder = DataFeederWavenet(dirs, B, rf, gc_enable=True, hp=hp)
                elif route == "host+prefetch":
                    feeder = PrefetchFeeder(DataFeederWavenet(dirs, B, rf, gc_enable=True, hp=hp))
                elif route == "resident":
                    index.rewind()
                    feeder = dev_feeder
                times = []
                t0 = time.perf_counter()
                for k in range(count):
                    batch = fixed if feeder is None else feeder.next_batch()
                    if k == 0 and feeder is not None:
                        first[route] = [np.asarray(x.cpu() if torch.is_tensor(x) else x).tobytes() for x in batch]
                    float(tr.step(*batch).item())
                    t1 = time.perf_counter()
                    times.append(t1 - t0)
                    t0 = t1
                if route == "host+prefetch":
                    feeder.close()
                return times
            run("floor", 4); run("resident", 2)                     # code objects, rocBLAS, pinned memory
            res = {n: [] for n in ROUTES}
            for _ in range(a.rounds):
                for n in ROUTES:
                    res[n].append(run(n, a.batches))
            assert first["parent"] == first["host+prefetch"] == first["resident"], "the routes' first batches differ"
            # device events: next_batch() on the device (copy of the picks + the launch), and the launch alone on picks already there
            index.rewind()
            np.random.seed(1234)
            ev_feed, ev_launch = [], []
            for _ in range(a.batches):
                ex, st, _ = index.next_picks()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); out = dev_feeder.stage(ex, st); e1.record(); sync()
                ev_feed.append(e0.elapsed_time(e1))
                pk = np.ascontiguousarray(np.stack([ex, st], axis=1))
                pk_dev = torch.from_numpy(pk).cuda()
                sync()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                crop_stage(dev_feeder.audio_pool, dev_feeder.mel_pool, dev_feeder.table, dev_feeder.table_dev, pk, pk_dev, index.max_frames, index.hop_size,
                           index.num_mels, out=out)
                e1.record(); sync()
                ev_launch.append(e0.elapsed_time(e1))
            mean = {n: float(np.mean([np.mean(x) for x in res[n]])) for n in ROUTES}
            spread = max(abs(np.mean(res[n][0]) - np.mean(res[n][-1])) for n in ROUTES)
            crop_bytes = 4 * 2 * B * index.max_frames * (index.hop_size + index.num_mels)
            lines += ["", "B = %d x %d samples (%d frames)   route %s" % (B, tr.sample_size, index.max_frames, tr.route()),
                      "pack: %d examples, %d bytes (%.3f GB) read and packed in %.2f s, uploaded in %.2f s" % (index.n_examples, index.packed_bytes, index.packed_bytes / 1e9, t_pack, t_upload),
                      "%-16s %s" % ("route", "  ".join("round %d mean / median" % (k + 1) for k in range(a.rounds)))]
            for n in ROUTES:
                lines.append("%-16s %s" % (n, "  ".join("%9.5f / %9.5f   " % (np.mean(x), np.median(x)) for x in res[n])))
            inside = lambda d: " (inside the spread between rounds)" if abs(d) <= spread else ""
            lines += ["largest difference between a route's rounds: %.5f s -- differences below it are not measured" % spread,
                      "(a) parent - floor          %+9.5f s per step = %.1f %% of the parent's step%s" % (mean["parent"] - mean["floor"], 100 * (mean["parent"] - mean["floor"]) / mean["parent"], inside(mean["parent"] - mean["floor"])),
                      "(b) host+prefetch - floor   %+9.5f s%s" % (mean["host+prefetch"] - mean["floor"], inside(mean["host+prefetch"] - mean["floor"])),
                      "(c) resident - floor        %+9.5f s%s" % (mean["resident"] - mean["floor"], inside(mean["resident"] - mean["floor"])),
                      "resident against parent     %+9.5f s per step (%.1f %% of the parent's)%s" % (mean["resident"] - mean["parent"], 100 * mean["resident"] / mean["parent"], inside(mean["resident"] - mean["parent"])),
                      "resident <= parent outside the spread: %s" % ("yes" if mean["parent"] - mean["resident"] > spread else "NO: a finding, see DESIGN 3c-f"),
                      "device events over %d batches: next_batch() on the device (copy of %d bytes of picks + the crop launch) median %.4f ms, max %.4f ms; the launch alone median %.4f ms (%d bytes read + written, %.2f TB/s: bound by the launch)"
                      % (a.batches, 8 * B, np.median(ev_feed), np.max(ev_feed), np.median(ev_launch), crop_bytes, crop_bytes / (np.median(ev_launch) * 1e-3) / 1e12)]
            del tr, net, dev_feeder, index, fixed
            torch.cuda.empty_cache()
    if a.step_log:
        rows = [json.loads(l) for l in open(a.step_log) if l.startswith("{")]
        lines += ["", "WaveNetTrainer.step alone (scripts/train_bench.py, B = 64 x 7800, fixed device tensors; this build and the parent build, processes alternating), ms per step:"]
        for build in ("this", "parent"):
            v = [r["ms_per_step"] for r in rows if r.get("build") == build]
            if v:
                lines.append("  %-7s %s   median %.2f" % (build, " ".join("%.2f" % x for x in v), sorted(v)[len(v) // 2]))
    text = "\n".join(lines) + "\n"
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
