"""One rank of tests/test_train_tacotron_gpu.py::test_two_ranks_on_two_gpus: a four-step `train_tacotron` on the small hparams over the given
data directories, then `<out>.rank<RANK>.json` with the SHA-256 digest of the rank's final variables(), its step and its losses.  Run as
`python -m torch.distributed.run --nproc-per-node 2 tests/tacotron_two_ranks.py LOG_DIR OUT DIR1,DIR2` (one process per GPU, the launcher
bench.py --gpus 2 uses), or plainly with python for the one-rank run."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def small_hp():
    from tacotron_grad_cases import SMALL, hparams
    return hparams(max_iters=8, min_iters=1, min_tokens=2, fft_size=256, hop_size=64, win_size=256, griffin_lim_iters=2, initial_phase_step=4,
                   tacotron_initial_learning_rate=1e-3, decay_learning_rate_mode=1, **SMALL)


def digest(variables):
    h = hashlib.sha256()
    for name in sorted(variables):
        h.update(name.encode() + b"\0" + variables[name].tobytes())
    return h.hexdigest()


def run(log_dir, out, data_paths, steps=4):
    from twvk_amd import train_tacotron
    lines = []
    # intervals beyond the run: no checkpoint, summary or test output -- the variables are what is compared
    res = train_tacotron.main(["--log_dir", log_dir, "--data_paths", data_paths, "--batch_size", "3", "--random_seed", "7", "--num_steps", str(steps),
                               "--checkpoint_interval", "1000", "--test_interval", "1000", "--summary_interval", "1000"], hp=small_hp(), log=lines.append)
    rank = int(os.environ.get("RANK", "0"))
    record = {"rank": rank, "world": int(os.environ.get("WORLD_SIZE", "1")), "step": res["step"], "losses": res["losses"], "model_dir": res["model_dir"],
              "digest": digest(res["trainer"].variables()), "peer_failure": bool(res["trainer"].peer_failure())}
    with open("%s.rank%d.json" % (out, rank), "w") as f:
        json.dump(record, f)
    return record


if __name__ == "__main__":
    run(sys.argv[1], sys.argv[2], sys.argv[3])
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        dist.destroy_process_group()
