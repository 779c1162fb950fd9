#!/usr/bin/env python
"""The record of the manual-attention pass against its float64 checker: runs the checker cases of
tests/test_tacotron_manual_gpu.py themselves, so the record cannot drift from what the tests hold, and keeps what they print before they
assert -> profiles/tacotron_manual_attention_parity.txt.  Needs the GPU."""
import argparse, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tacotron_manual_attention_parity.txt"))
    args = ap.parse_args()
    import torch
    import twvk_amd
    assert torch.cuda.is_available(), "the record needs the GPU"
    head = ["Tacotron passes with caller-supplied alignments (Tacotron.infer_manual) against the float64 checker tests/torch_manual_attention_ref.py:",
            "what tests/test_tacotron_manual_gpu.py::test_manual_pass_against_the_float64_checker prints before it asserts (scripts/tacotron_manual_parity.py).",
            "rel distance = max |kernel - checker| / max |checker|; random alignments whose rows sum to 1 over the valid positions, 0.5e-3 .. 1.5e-3 past",
            "the lengths; the emitted alignments are compared bit for bit.  The bar is RTOL of tests/test_attention_types_gpu.py.",
            "library %s on %s" % (twvk_amd._lib.lib().twv_version().decode(), torch.cuda.get_device_name(0)), ""]
    run = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_tacotron_manual_gpu.py"), "-m", "gpu", "-q", "-s",
                          "-k", "float64_checker", "-p", "no:cacheprovider"], capture_output=True, text=True, cwd=ROOT)
    with open(args.out, "w") as fh:
        fh.write("\n".join(head) + run.stdout)
    print(run.stdout[-3000:])
    return run.returncode


if __name__ == "__main__":
    sys.exit(main() or 0)
