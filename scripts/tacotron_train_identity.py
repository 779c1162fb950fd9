#!/usr/bin/env python
"""Bit identity of what existed before the training step, one build against another: `infer`, `forward_targets` (free-running and
teacher-forced) and `loss_gradients` on every case of tests/tacotron_cbhg_grad_cases.py, `decoder_grad` on every case of
tests/tacotron_grad_cases.py (bah_mon_norm and bah_mon), and one `TacotronTrainer.step` with the
constructor's defaults, and one in the training graph, on the whole-model cases of tests/tacotron_train_cases.py (the losses and every
variable after the update).

    python scripts/tacotron_train_identity.py --root PARENT_CHECKOUT --dump parent.json      # a checkout WITH its built library
    python scripts/tacotron_train_identity.py --dump new.json
    python scripts/tacotron_train_identity.py --compare parent.json new.json --out profiles/tacotron_train_identity.txt

A dump holds, per case and output tensor, its element count and the SHA-256 of its bytes; two dumps made on one MI355X are compared
digest by digest.  The dump needs the GPU."""
import argparse, hashlib, json, os, sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dump(root, path):
    sys.path.insert(0, os.path.join(HERE, "tests")); sys.path.insert(0, root)
    import numpy as np
    import twvk_amd
    assert os.path.dirname(os.path.dirname(os.path.abspath(twvk_amd.__file__))) == root, twvk_amd.__file__
    from twvk_amd.tacotron import Tacotron
    from tacotron_cbhg_grad_cases import CASES, host_case
    import torch
    torch_of = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    digest = lambda t: (int(t.numel()), hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()).hexdigest())
    out = {"library": twvk_amd._lib.lib().twv_version().decode(), "entries": {}}
    for name in sorted(CASES):
        h = host_case(name)
        m = Tacotron(h.hp, num_speakers=h.speakers)
        m.load_weights(h.w)
        passes = [("infer", lambda: m.infer(h.tok, h.ln, h.spk))]
        if h.forced:
            passes += [("forward_targets free-running", lambda: m.forward_targets(h.tok, h.ln, h.spk, h.tgt, teacher_forced=False)),
                       ("forward_targets teacher-forced", lambda: m.forward_targets(h.tok, h.ln, h.spk, h.tgt, teacher_forced=True))]
        for label, run in passes:
            out["entries"]["%s %s" % (label, name)] = {k: digest(t) for k, t in zip(("mel", "linear", "alignments"), run())}
        if h.forced:        # (the last pass above is the teacher-forced one)
            out["entries"]["loss_gradients %s" % name] = {k: digest(t) for k, t in sorted(m.loss_gradients(h.lin_tgt, h.coeff).items())}
    # decoder_grad alone on every case of tests/tacotron_grad_cases.py (both monotonic types: G-bah_mon is the other one; masks where the
    # case has them): every decoder-side gradient, d_memory, d_init and the recorded mel
    import tacotron_grad_cases as GC
    for name in sorted(GC.CASES):
        c = GC.HostCase(name)
        m = Tacotron(c.hp, num_speakers=2)
        m.load_weights(c.w)
        m.forward_targets(c.tok, c.ln, c.spk, c.tgt, teacher_forced=True)
        out["entries"]["decoder_grad %s (%s)" % (name, c.at)] = {k: digest(t) for k, t in sorted(m.decoder_grad(c.d_mel, c.masks).items())}
    # one TacotronTrainer step with the constructor's defaults (the evaluation graph) and one with training=True on the whole-model cases of tests/tacotron_train_cases.py:
    # the losses and every variable after the update
    from tacotron_train_cases import WHOLE, whole_case
    from twvk_amd.tacotron_train import TacotronTrainer
    for name in sorted(WHOLE):
        h = whole_case(name)
        for label, kw in (("TacotronTrainer.step", {}), ("TacotronTrainer(training=True, seed=7).step", dict(training=True, seed=7))):
            m = Tacotron(h.hp, num_speakers=h.speakers)
            m.load_weights(h.w)
            t = TacotronTrainer(m, **kw)
            losses = t.step(h.tok, h.ln, h.spk, h.tgt, h.lin_tgt, h.coeff)
            entry = {k: digest(torch_of(v)) for k, v in sorted(t.variables().items())}
            entry["losses"] = (4, hashlib.sha256(repr(sorted(losses.items())).encode()).hexdigest())
            out["entries"]["%s %s" % (label, name)] = entry
    with open(path, "w") as fh:
        json.dump(out, fh)
    print("wrote", path, len(out["entries"]), "entries,", out["library"])


def compare(a_path, b_path, out_path):
    a, b = json.load(open(a_path)), json.load(open(b_path))
    lines = ["Bit identity of `infer`, `forward_targets`, `loss_gradients`, `decoder_grad` and `TacotronTrainer.step` in both graphs, parent build against this tree: every case of",
             "tests/tacotron_cbhg_grad_cases.py CASES, tests/tacotron_grad_cases.py CASES and tests/tacotron_train_cases.py WHOLE (scripts/tacotron_train_identity.py).  Two processes on one MI355X, each the Python package and the",
             "library of one commit; every output tensor's bytes compared by SHA-256.  The condition: 0 differing tensors everywhere.",
             "parent: %s" % a["library"], "new:    %s" % b["library"], ""]
    tensors = elements = differing = 0
    assert set(a["entries"]) == set(b["entries"]), set(a["entries"]) ^ set(b["entries"])
    for key in a["entries"]:
        ea, eb = a["entries"][key], b["entries"][key]
        assert set(ea) == set(eb), (key, set(ea) ^ set(eb))
        bad = [k for k in ea if ea[k] != eb[k]]
        n = sum(v[0] for v in ea.values())
        tensors += len(ea); elements += n; differing += len(bad)
        lines.append("%-62s %4d tensors %10d elements  %s" % (key, len(ea), n, "identical" if not bad else "DIFFERENT: " + ", ".join(bad)))
    lines += ["", "%d tensors, %d elements; tensors with a differing bit: %d" % (tensors, elements, differing)]
    text = "\n".join(lines) + "\n"
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(text)
    print(text)
    return differing


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--dump", default=None)
    ap.add_argument("--compare", nargs=2, default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.compare:
        sys.exit(1 if compare(args.compare[0], args.compare[1], args.out) else 0)
    dump(os.path.abspath(args.root), args.dump)
