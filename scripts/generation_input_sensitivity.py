#!/usr/bin/env python
"""How much of the network does sample equality see?  CPU only: the oracle against itself.

For each kind of input of the generation tests -- the plain ones the suite used before, and those of tests/sensitive_inputs.py --
one weight tensor at a time is scaled by float32(1 + 2^-10) and the oracle is run again on the same inputs: the table says how
many samples change and at which step the first one does.  tests/test_generation_inputs_cpu.py asserts the essentials of this
table; this script prints all of it, together with the clamp share of the two committed fixtures.

    python scripts/generation_input_sensitivity.py [profiles/generation_input_sensitivity.txt]"""
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import oracle as O                      # noqa: E402
import sensitive_inputs as SI                       # noqa: E402
import test_generation_inputs_cpu as G              # noqa: E402

OLD = [("old: MoL plain, unshifted, scale 0.05", dict(scalar=True, scale=0.05, shift=False, knife_edge=False)),
       ("old: MoL plain, unshifted, scale 0.10, S=512 (test_generate_variants)", dict(scalar=True, scale=0.1, S=512, shift=False, knife_edge=False)),
       ("old: MoL plain, unshifted, scale 0.20", dict(scalar=True, scale=0.2, shift=False, knife_edge=False)),
       ("shift only: MoL plain uniforms, shifted head, scale 0.05", dict(scalar=True, scale=0.05, knife_edge=False)),
       ("old: one-hot plain, scale 0.05", dict(scalar=False, scale=0.05, knife_edge=False, dil=[1, 2, 4, 8, 16], T=50, direct_lc=True)),
       ("old: one-hot plain, scale 0.12", dict(scalar=False, scale=0.12, knife_edge=False, dil=[1, 2, 4, 8, 16], T=50, direct_lc=True)),
       ("old: one-hot plain, scale 0.30", dict(scalar=False, scale=0.3, knife_edge=False, dil=[1, 2, 4, 8, 16], T=50, direct_lc=True))]


def short(label):
    return label.replace("wavenet/", "").replace("dilated_stack/", "").replace("dilation_layer/", "")


def report(out, title, kw):
    t0 = time.time()
    c = G.Case(O, **kw)
    rows = c.table()
    n = c.want.size
    out.write("\n== %s\n" % title)
    out.write("   %d layers, B = %d, T = %d (%d samples); built and swept in %.1f s\n" % (c.d.n_layers, c.B, c.T, n, time.time() - t0))
    if c.scalar:
        out.write("   oracle's samples equal to +-1: %.1f %%; distinct values: %.0f %%; draws with an edge: %d of %d\n"
                  % (100 * SI.clamp_share(c.want), 100.0 * len(np.unique(c.want)) / n, c.n_edges, n))
    else:
        out.write("   distinct classes: %d; draws with an edge: %d of %d\n" % (len(np.unique(c.want)), c.n_edges, n))
    live = [r for r in rows if not r[1]]
    changed = sorted(r[2] for r in live)
    out.write("   mutants: %d (+ %d exempt: the last layer's dense); survivors: %d; changed samples min / median / max: %d / %d / %d\n"
              % (len(live), len(rows) - len(live), sum(1 for r in live if r[2] == 0), changed[0], changed[len(changed) // 2], changed[-1]))
    # one row per tensor class: the layers of the stack folded into min / median / max
    classes = {}
    for label, exempt, k, first in rows:
        key = re.sub(r"layer\d+/", "layer*/", short(label)) + (" (last layer: exempt)" if exempt else "")
        classes.setdefault(key, []).append((k, first))
    out.write("   %-58s %7s %22s %11s\n" % ("tensor class scaled by (1 + 2^-10)", "tensors", "changed min/med/max", "first step"))
    for key, v in classes.items():
        ks = sorted(k for k, _ in v)
        firsts = [f for _, f in v if f is not None]
        out.write("   %-58s %7d %22s %11s\n" % (key, len(v), "%d / %d / %d" % (ks[0], ks[len(ks) // 2], ks[-1]),
                                               "-" if not firsts else "%d..%d" % (min(firsts), max(firsts))))


def fixtures(out):
    g = np.load(os.path.join(ROOT, "tests", "golden", "restatement_wavenet_mol_small.npz"))
    s = g["samples"]
    out.write("\n== committed fixtures (left as they are)\n")
    out.write("   restatement_wavenet_mol_small.npz: scale %.2f, %d samples, %.1f %% equal to +-1\n" % (float(g["scale"]), s.size, 100 * SI.clamp_share(s)))
    g = np.load(os.path.join(ROOT, "tests", "golden", "restatement_wavenet_mulaw_small.npz"))
    for k in ("samples_t10", "samples_t08"):
        out.write("   restatement_wavenet_mulaw_small.npz %s: scale %.2f, %d class ids, %d distinct, plain uniforms\n"
                  % (k, float(g["scale"]), g[k].size, len(np.unique(g[k]))))


def main(path=None):
    O.build()
    out = open(path, "w") if path else sys.stdout
    out.write("generation inputs x tensor -> samples of the ORACLE that change when that tensor is scaled by float32(1 + 2^-10)\n")
    out.write("(scripts/generation_input_sensitivity.py; CPU only; stack %s unless stated, S = %d)\n" % (G.DIL, G.S))
    for title, kw in OLD:
        report(out, title, kw)
    for name, kw in G.CONFIGS:
        report(out, "new: " + name, kw)
    fixtures(out)
    if path:
        out.close()


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
