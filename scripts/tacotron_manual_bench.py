#!/usr/bin/env python
"""Pass times around caller-supplied alignments (Tacotron.infer_manual), for profiles/tacotron_manual_attention_bench.txt.

One process measures one build of the tree and prints one JSON line: median ms of `--passes` single `infer` passes at B = 8 and B = 32
(101 tokens, 200 decoder steps, post-CBHG + linear on: the workload and weights of scripts/tacotron_bench.py) and -- where the tree has
them -- at B = 32 the manual pass (fed the alignments of that `infer`, transposed on the device), `infer` forced onto the split kernel
(decoder_groups = 8, the kernel a manual pass runs on) beside `infer` at the default, and the alignment edit kernel's four modes at
(32, 101, 200) by device events.

`--root DIR` is a checkout WITH its built library (the Python package and libtwv_amd.so of one commit are loaded together), as in
scripts/tacotron_targets_bench.py.  Alternate processes of the parent's root and this tree's on one box, labels A1 B1 A2 B2 ...:
    python scripts/tacotron_manual_bench.py --root PARENT --label A1 >> lines.txt; python scripts/tacotron_manual_bench.py --label B1 >> lines.txt; ...
    python scripts/tacotron_manual_bench.py --summarise lines.txt [--isa ISA_DIFF.txt] > profiles/tacotron_manual_attention_bench.txt
`--isa` appends the output of scripts/kernel_isa_diff.py (parent against this tree) for the sources the change touched.
The manual pass has no bar (nobody measured one before): its number is recorded.  The bar is on `infer`: this tree minus the parent inside
the parent's own run-to-run spread of the same visit."""
import argparse, json, os, sys, time

EDIT_CALLS = 20


def summarise(path, isa):
    import numpy as np
    rows = [json.loads(l) for l in open(path) if l.strip().startswith("{")]
    A = [r for r in rows if r["label"].startswith("A")]; B = [r for r in rows if r["label"].startswith("B")]
    med = lambda v: float(np.median(v))
    out = ["Tacotron passes with caller-supplied alignments, and `infer` against the parent build: processes alternating A1 B1 A2 B2 ... (A = parent",
           "build, B = this tree) on one MI355X, each figure the median of %d single passes (scripts/tacotron_manual_bench.py; 101 tokens, 200 decoder"
           % rows[0].get("passes", 15), "steps, post-CBHG + linear on; wall clock around pass + synchronize).", ""]
    out.append("B = 32, this tree (ms, one figure per process):")
    for k, what in (("manual_b32_ms", "infer_manual (%s)" % B[0].get("manual_kernel", "?")), ("split_b32_ms", "infer, decoder_groups = 8 (%s)" % B[0].get("split_kernel", "?")),
                    ("infer_b32_ms", "infer, default (%s)" % B[0].get("kernel_b32", "?"))):
        v = [r[k] for r in B if k in r]
        out.append("  %-46s %s   median %.4f" % (what, " ".join("%.4f" % x for x in v), med(v)))
    m, s, d = (med([r[k] for r in B]) for k in ("manual_b32_ms", "split_b32_ms", "infer_b32_ms"))
    out += ["  the manual pass against the mechanism's pass on the same kernel: %+.4f ms (%+.2f %%); against the default route: %+.4f ms (%+.2f %%)"
            % (m - s, 100 * (m - s) / s, m - d, 100 * (m - d) / d),
            "  (no bar on the manual pass: a first measurement.  It skips the query stage's tiles and exchange, the score and its exchange and the",
            "  recurrence, and reads one row of T_in floats per step and workgroup instead.)", ""]
    out.append("alignment edit kernel at (32, 101, 200), device events around one launch, median of %d (us): %s" % (
        EDIT_CALLS, "  ".join("mode %d: %.1f" % (i, med([r["edit_us"][i] for r in B])) for i in range(4))))
    out.append("  (2.6 MB read + 2.6 MB written by 4 x 32 workgroups of 32 encoder rows; modes 1 and 3 read the rows once more for the argmax.  Once per")
    out.append("  batch, beside a pass of milliseconds: not tuned further)")
    out.append("")
    out.append("`infer` against the parent build (the bar: B - A of the medians inside the parent's own spread, max - min over its processes):")
    for k in ("infer_b8_ms", "infer_b32_ms"):
        a = [r[k] for r in A]; b = [r[k] for r in B]
        out.append("%-13s %-22s A: %s   median %.4f  spread %.4f" % (k, "(" + A[0]["kernel_" + k.split("_")[1]] + ")", " ".join("%.4f" % v for v in a), med(a), max(a) - min(a)))
        out.append("%-13s %-22s B: %s   median %.4f  spread %.4f" % ("", "", " ".join("%.4f" % v for v in b), med(b), max(b) - min(b)))
        dd = med(b) - med(a)
        out.append("%-36s B - A of the medians: %+.4f ms (%+.2f %%); the parent's own spread: %.4f ms -> %s"
                   % ("", dd, 100 * dd / med(a), max(a) - min(a), "inside" if dd <= max(a) - min(a) else "OUTSIDE"))
        out.append("")
    if isa:
        out += ["scripts/kernel_isa_diff.py, parent against this tree (twv_tacotron.hip, twv_tacotron_feed.hip; the kernels marked NEW are the change,",
                "`a -> b` pairs a kernel with the instantiation that gained a template parameter):", ""] + open(isa).read().rstrip("\n").split("\n")
    return "\n".join(out) + "\n"


def measure(args):
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import numpy as np, torch
    import twvk_amd
    assert os.path.dirname(os.path.dirname(os.path.abspath(twvk_amd.__file__))) == root, twvk_amd.__file__
    from twvk_amd.tacotron import Tacotron
    from tacotron_targets_bench import random_tensors

    def med(fn):
        for _ in range(3): fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.passes):
            t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts))

    hp = twvk_amd.default_hparams()
    m = Tacotron(hp, num_speakers=2)
    m.load_weights(random_tensors(m.specs))
    out = {"label": args.label, "passes": args.passes}
    for N in (8, 32):
        rng = np.random.RandomState(1); T = 101
        tok = rng.randint(2, 80, (N, T)).astype(np.int32); tok[:, -1] = 1
        ln = np.full(N, T, np.int32); spk = (np.arange(N) % 2).astype(np.int32)
        out["kernel_b%d" % N] = m.decoder_kernel_name(N, T)
        out["infer_b%d_ms" % N] = med(lambda: m.infer(tok, ln, spk))
    if hasattr(m, "infer_manual"):                                   # (N = 32 from here on)
        al = m.infer(tok, ln, spk)[2]
        man = m.edit_alignments(al, 0)
        out["manual_kernel"] = m.manual_kernel_name(N, T)
        out["manual_b32_ms"] = med(lambda: m.infer_manual(tok, ln, spk, man))
        m.set_option("decoder_groups", 8)
        out["split_kernel"] = m.decoder_kernel_name(N, T)
        out["split_b32_ms"] = med(lambda: m.infer(tok, ln, spk))
        m.set_option("decoder_groups", 0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        out["edit_us"] = []
        for mode in range(4):
            for _ in range(3): m.edit_alignments(al, mode)
            ts = []
            for _ in range(EDIT_CALLS):
                torch.cuda.synchronize(); e0.record(); m.edit_alignments(al, mode); e1.record(); torch.cuda.synchronize(); ts.append(e0.elapsed_time(e1) * 1e3)
            out["edit_us"].append(float(np.median(ts)))
    print(json.dumps(out))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--passes", type=int, default=15); ap.add_argument("--label", default="")
    ap.add_argument("--summarise", default=None); ap.add_argument("--isa", default=None)
    args = ap.parse_args(argv)
    if args.summarise:
        sys.stdout.write(summarise(args.summarise, args.isa))
    else:
        measure(args)


if __name__ == "__main__":
    main()
