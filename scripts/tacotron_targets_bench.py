#!/usr/bin/env python
"""Pass times of one build of the tree for an A/B of two commits: median ms of `--passes` single `infer` passes at B = 8 and B = 32
(the workload and weights of scripts/tacotron_bench.py), and -- where the tree has them -- of the free-running and the teacher-forced
`forward_targets` pass over the same 200 steps; `--loss`: twv_tacotron_loss at B = 32 x 1000 x 1025 beside its two-read byte floor.

`--root DIR` is a checkout WITH its built library: the Python package and libtwv_amd.so of one commit are loaded together (a library
of the parent commit lacks symbols the newer _lib.py declares, so scripts/ab_two_builds.sh's swap of the .so alone does not serve here).
Alternate processes of the two roots on one box (boxes differ by 0.5-1 %); `--summarise FILE` condenses the collected JSON lines (labels
A<n> = parent, B<n> = this tree) into the table of profiles/tacotron_targets_ab.txt."""
import argparse, json, os, sys, time

LOSS_CALLS = 20


def summarise(path):
    import numpy as np
    rows = [json.loads(l) for l in open(path) if l.strip().startswith("{")]
    A = [r for r in rows if r["label"].startswith("A")]; B = [r for r in rows if r["label"].startswith("B")]
    out = ["Tacotron pass times, parent build (A) against this tree (B): processes alternating A1 B1 A2 B2 ... on one MI355X, each the median of",
           "%d single passes per figure (scripts/tacotron_targets_bench.py; B = 8 / 32, 101 tokens, 200 decoder steps, post-CBHG + linear on)."
           % rows[0].get("passes", 15), ""]
    for k in ("infer_b8_ms", "infer_b32_ms"):
        a = [r[k] for r in A]; b = [r[k] for r in B]
        out.append("%-13s %-20s A: %s   median %.4f  spread (max - min) %.4f" % (k, "(" + A[0]["kernel_" + k.split("_")[1]] + ")", " ".join("%.4f" % v for v in a), np.median(a), max(a) - min(a)))
        out.append("%-13s %-20s B: %s   median %.4f  spread (max - min) %.4f" % ("", "", " ".join("%.4f" % v for v in b), np.median(b), max(b) - min(b)))
        d = np.median(b) - np.median(a)
        out.append("%-34s B - A of the medians: %+.4f ms (%+.2f %%); the parent's own spread: %.4f ms -> %s" % ("", d, 100 * d / np.median(a), max(a) - min(a), "inside" if d <= max(a) - min(a) else "OUTSIDE"))
        out.append("")
    out.append("forward_targets over the same 200 steps (this tree only; ms, per process):")
    for k in ("free_b8_ms", "forced_b8_ms", "free_b32_ms", "forced_b32_ms"):
        b = [r[k] for r in B if k in r]
        out.append("%-14s %s   median %.4f" % (k, " ".join("%.4f" % v for v in b), np.median(b)))
    for r in B:
        if "loss_us_median" in r:
            byt = r["loss_bytes"]
            out += ["", "twv_tacotron_loss at B = 32 x 1000 frames x (1025 + 80) bins, prioritize_loss on (two kernels, stream-ordered scratch; HIP events around the call):",
                    "median %.1f us, min %.1f us of %d calls; two reads of the inputs = %.1f MB -> %.2f TB/s at the median (byte floor at 8 TB/s: %.1f us)"
                    % (r["loss_us_median"], r["loss_us_min"], r.get("loss_calls", LOSS_CALLS), byt / 1e6, byt / r["loss_us_median"] / 1e6, byt / 8e12 * 1e6)]
    return "\n".join(out) + "\n"


def random_tensors(specs, seed=0):
    """the weights of scripts/tacotron_bench.py (that script runs on import, so its function cannot be imported)"""
    import numpy as np
    rng = np.random.RandomState(seed); t = {}
    for n, shp in specs:
        if n.endswith("batch_normalization"):
            c = shp[1]; t[n] = np.stack([np.ones(c), np.zeros(c), np.zeros(c), np.ones(c)]).astype(np.float32)
        elif n.endswith("gates/bias"): t[n] = np.ones(shp, np.float32)
        elif n.endswith("T/bias"): t[n] = -np.ones(shp, np.float32)
        elif n.endswith("attention_g"): t[n] = np.array([np.sqrt(1.0 / 256)], np.float32)
        elif n.endswith("attention_score_bias"): t[n] = np.zeros(1, np.float32)
        else:
            fan = int(np.prod(shp[:-1])) if len(shp) > 1 else 1
            t[n] = (rng.randn(*shp) * (0.05 if len(shp) == 1 else min(0.5, 1.2 / np.sqrt(fan)))).astype(np.float32)
    return t


def measure(args):
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    import numpy as np, torch
    import twvk_amd
    assert os.path.dirname(os.path.dirname(os.path.abspath(twvk_amd.__file__))) == root, twvk_amd.__file__
    from twvk_amd.tacotron import Tacotron

    def med(fn):
        for _ in range(3): fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.passes):
            t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts)), float(np.min(ts))

    hp = twvk_amd.default_hparams()
    m = Tacotron(hp, num_speakers=2)
    m.load_weights(random_tensors(m.specs))
    out = {"label": args.label, "passes": args.passes}
    for N in (8, 32):
        rng = np.random.RandomState(1); T = 101
        tok = rng.randint(2, 80, (N, T)).astype(np.int32); tok[:, -1] = 1
        ln = np.full(N, T, np.int32); spk = (np.arange(N) % 2).astype(np.int32)
        out["kernel_b%d" % N] = m.decoder_kernel_name(N, T)
        out["infer_b%d_ms" % N], out["infer_b%d_min_ms" % N] = med(lambda: m.infer(tok, ln, spk))
        if hasattr(m, "forward_targets"):
            tg = torch.from_numpy(rng.uniform(-4, 4, (N, 1000, 80)).astype(np.float32)).cuda()
            out["forced_b%d_ms" % N], _ = med(lambda: m.forward_targets(tok, ln, spk, tg, teacher_forced=True))
            out["free_b%d_ms" % N], _ = med(lambda: m.forward_targets(tok, ln, spk, tg, teacher_forced=False))
    if args.loss:
        import ctypes as C
        L = twvk_amd._lib.lib()
        B, TO, M, F = 32, 1000, 80, 1025
        g = torch.Generator(device="cuda"); g.manual_seed(1)
        mel, mel_t = [torch.rand((B, TO, M), device="cuda", generator=g) for _ in range(2)]
        lin, lin_t = [torch.rand((B, TO, F), device="cuda", generator=g) for _ in range(2)]
        co = torch.ones(B, device="cuda"); o = torch.zeros(4, dtype=torch.float64, device="cuda")
        p = lambda t: C.c_void_p(t.data_ptr())
        def run(): twvk_amd._lib.check(L.twv_tacotron_loss(p(mel), p(lin), p(mel_t), p(lin_t), p(co), B, TO, M, F, 1, 24000.0, p(o), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        for _ in range(3): run()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ts = []
        for _ in range(LOSS_CALLS):
            e0.record(); run(); e1.record(); torch.cuda.synchronize(); ts.append(e0.elapsed_time(e1) * 1e3)
        out["loss_us_median"] = float(np.median(ts)); out["loss_us_min"] = float(np.min(ts)); out["loss_calls"] = LOSS_CALLS
        out["loss_bytes"] = 2.0 * B * TO * (F + M) * 4
        out["loss_values"] = [float(v) for v in o.cpu().numpy()]
    print(json.dumps(out))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--passes", type=int, default=15); ap.add_argument("--label", default="")
    ap.add_argument("--loss", action="store_true"); ap.add_argument("--summarise", default=None)
    args = ap.parse_args(argv)
    if args.summarise:
        sys.stdout.write(summarise(args.summarise))
    else:
        measure(args)


if __name__ == "__main__":
    main()
