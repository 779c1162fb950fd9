#!/usr/bin/env python
"""The record of the Tacotron training-mode tests.

    python scripts/tacotron_trainmode_parity.py --seeds          # host only: the first seed of every row of tests/tacotron_trainmode_cases.py
                                                                 # that meets the row's conditions, from the row's own seed on
    python scripts/tacotron_trainmode_parity.py                  # the GPU: every figure tests/test_tacotron_trainmode_gpu.py prints before it asserts
                                                                 # -> profiles/tacotron_trainmode_parity.txt

The second form runs the test file itself, so the record cannot drift from what the tests hold; the twenty-step run prints the device's
losses beside the float64 checker's own, which is run on the host first."""
import argparse, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def seeds(span):
    import tacotron_trainmode_cases as TC
    for name, row in sorted(TC.CASES.items()):
        for seed in range(row[-1], row[-1] + span):
            same, relu, gap = TC.HostCase(name, seed=seed).margins()
            print("%-22s seed %d: same branches %s, relu margin %.3e, pool gap %.3e" % (name, seed, same, relu, gap), flush=True)
            if same and relu > TC.MARGIN and gap > TC.MARGIN:
                break
    for name, row in sorted(TC.STEP_CASES.items()):
        for seed in range(row[-1], row[-1] + span):
            ok, fig = TC.step_conditions(TC.HostCase(name, seed=seed, table={name: row[:6] + (False, seed)}))
            print("%-22s seed %d: %s %s" % (name, seed, ok, fig), flush=True)
            if ok:
                break


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", action="store_true")
    ap.add_argument("--span", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tacotron_trainmode_parity.txt"))
    args = ap.parse_args()
    if args.seeds:
        return seeds(args.span)
    import tacotron_trainmode_cases as TC
    name = sorted(TC.TWENTY_CASES)[0]
    l64, g1 = TC.checker_trajectory(name)               # (the checker first, on the host)
    import torch
    import twvk_amd
    assert torch.cuda.is_available(), "the record needs the GPU"
    head = ["Tacotron training mode against the float64 checker (tests/torch_tacotron_trainmode_ref.py): what tests/test_tacotron_trainmode_gpu.py prints",
            "before it asserts (scripts/tacotron_trainmode_parity.py).  e_hip / e_t32: the device's and the float32 autograd run's distance from float64,",
            "relative to the tensor's maximum; the bar is e_hip <= max(8 e_t32, 5e-6).",
            "library %s on %s" % (twvk_amd._lib.lib().twv_version().decode(), torch.cuda.get_device_name(0)), "",
            "float64 checker, twenty training-mode steps on %s, run on the host: loss %.7f -> %.7f, sum |gradient| at the last step %.3f" % (name, l64[0], l64[-1], g1), ""]
    run = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_tacotron_trainmode_gpu.py"), "-m", "gpu", "-q", "-s", "-p", "no:cacheprovider"],
                         capture_output=True, text=True, cwd=ROOT)
    with open(args.out, "w") as fh:
        fh.write("\n".join(head) + run.stdout)
    print(run.stdout[-3000:])
    return run.returncode


if __name__ == "__main__":
    sys.exit(main() or 0)
