"""The Tacotron training loop on the device: feeder batches of varying shape through the new route (staged device tensors,
reshaped handles, reserved workspaces) against TacotronTrainer.step on host-padded numpy batches with newly created handles; the
data-parallel arithmetic on one GPU through the replaceable reduction; and `train_tacotron` itself on a small synthetic data set."""
import functools
import json
import os

import numpy as np
import pytest

from helpers import first_mismatch, same_outputs
from tacotron_feed_cases import write_directories
from tacotron_grad_cases import SMALL, hparams
from tacotron_train_cases import TWENTY_LR0, TWENTY_MODE, TWENTY_STEPS, whole_case
from test_tacotron_train_gpu import STEP_ATOL, STEP_LR0

pytestmark = pytest.mark.gpu
MAX_ITERS = 8


def _hp(**kw):
    """SMALL with a short utterance filter and a small Griffin-Lim geometry (num_freq = 129 = fft_size / 2 + 1)"""
    return hparams(max_iters=MAX_ITERS, min_iters=1, min_tokens=2, fft_size=256, hop_size=64, win_size=256, griffin_lim_iters=2, initial_phase_step=4,
                   **dict(SMALL, **kw))


@functools.lru_cache(maxsize=None)
def _weights():
    import torch_attention_ref as AR
    from twvk_amd.tacotron import tacotron_specs
    return AR.random_tensors(tacotron_specs(_hp(), 2), seed=91)


def _trainer(training, hp=None, w=None, **kw):
    from twvk_amd.tacotron import Tacotron
    from twvk_amd.tacotron_train import TacotronTrainer
    m = Tacotron(hp or _hp(tacotron_initial_learning_rate=1e-3, decay_learning_rate_mode=1), num_speakers=2)
    m.load_weights(_weights() if w is None else w)
    return TacotronTrainer(m, training=training, seed=5, **kw)


# ---------------------------------------------------------------- the loop against the step as it was
@pytest.mark.parametrize("training", [False, True])
def test_eight_feeder_batches_through_the_new_route_equal_the_step_on_padded_batches(tmp_path, training):
    """the yardstick is TacotronTrainer.step on prepare_batch's numpy arrays with _drop_grad_handles() before each step: handles created
    at every shape, padding on the host.  After every step the losses are equal and variables() are equal bit for bit."""
    from twvk_amd.tacotron_feed import BatchStager, DataFeederTacotron, prepare_batch, staged_batches
    hp = _hp()
    dirs = write_directories(tmp_path, hp, speakers=2, per_speaker=12, seed=3, frames=(6, 34), tokens=(3, 12))
    feeders = [DataFeederTacotron(dirs, hp, 3, 2, "train", random_seed=9) for _ in range(2)]
    new, old = _trainer(training), _trainer(training)
    new.model.reserve_gradients(3, 12, MAX_ITERS)
    reserved = {k: e[2].data_ptr() for k, e in new.model._grad_cache.items()}
    stager = BatchStager(new.device, hp.num_mels, hp.num_freq)
    shapes = set()
    for k, (examples, batch) in enumerate(staged_batches(feeders[0], stager, count=8, prefetch=True)):
        got = new.step(batch["inputs"], batch["input_lengths"], batch["speaker_id"], batch["mel_targets"], batch["linear_targets"], batch["loss_coeff"])
        same = feeders[1].next_examples()
        assert [(ex["speaker_id"], ex["name"]) for ex in examples] == [(ex["speaker_id"], ex["name"]) for ex in same]
        host = prepare_batch(same, hp.reduction_factor)
        old.model._drop_grad_handles()
        want = old.step(host["inputs"], host["input_lengths"], host["speaker_id"], host["mel_targets"], host["linear_targets"], host["loss_coeff"])
        assert got == want and np.isfinite(list(got.values())).all(), (k, got, want)
        same_outputs(old.variables(), new.variables(), "step %d" % (k + 1))
        assert first_mismatch(batch["mel_targets"].cpu().numpy(), host["mel_targets"]) is None
        shapes.add((host["inputs"].shape[1], host["mel_targets"].shape[1]))
    assert len(shapes) >= 4, shapes                             # (the batches did vary in shape)
    assert new.global_step == old.global_step == 8
    assert {k: e[2].data_ptr() for k, e in new.model._grad_cache.items()} == reserved          # no workspace was allocated again


# ---------------------------------------------------------------- data-parallel arithmetic on one GPU
def _batches():
    h = whole_case("C-length-one")
    a = (h.tok, h.ln, h.spk, h.tgt, h.lin_tgt, 8.0 * h.coeff)                  # (x 8: the gradient's norm above the clip norm)
    b = (h.tok, h.ln, h.spk, (0.5 * h.tgt).astype(np.float32), (0.5 * h.lin_tgt + 0.1).astype(np.float32), 8.0 * h.coeff)
    hp = hparams(max_iters=8, **dict(SMALL, tacotron_initial_learning_rate=STEP_LR0, decay_learning_rate_mode=1))
    return h, hp, a, b


@pytest.mark.parametrize("training", [False, True])
def test_two_ranks_arithmetic_through_the_reduction_callable(training):
    """two trainers with equal weights and different batches; the second one's buffer reaches the first through the reduction callable.
    The first trainer's variables: within STEP_ATOL of float64 clip + Adam fed the mean of the two device gradients; its moving
    statistics: within 1e-6 of the float64 formula at the mean of the two ranks' statistics; a step with the failure flag set moves nothing."""
    import torch_tacotron_speaker_grad_ref as SG
    import torch_tacotron_trainmode_ref as TM
    h, hp, batch_a, batch_b = _batches()
    box = {}

    def capture(flat, group):
        box["peer"] = flat.clone()
        return 1

    def add_peer(flat, group):
        box["own"] = flat.clone()
        flat.add_(box["peer"])
        return 2
    peer = _trainer(training, hp, h.w, allreduce=capture)
    peer.step(*batch_b)
    first = _trainer(training, hp, h.w, allreduce=add_peer)
    before = first.variables()
    n = first.n_variables
    out = first.step(*batch_a)
    assert first.global_step == 1 and not first.peer_failure() and np.isfinite(out["loss"])
    own, other = box["own"].cpu().numpy(), box["peer"].cpu().numpy()
    assert own.size == other.size == first._gbuf.numel() and own[n] == other[n] == 0.0
    assert first_mismatch(own[:n], other[:n]) is not None
    # a third trainer alone on the first batch: the same unclipped gradient (and statistics) the first one put into the reduction
    alone = _trainer(training, hp, h.w)
    alone.loss_and_gradients(*batch_a)
    assert first_mismatch(alone.grads.cpu().numpy(), own[:n]) is None
    mean = ((own.astype(np.float64) + other.astype(np.float64)) / 2.0)
    raw = {k: mean[off:off + int(np.prod(shp))].reshape(shp) for k, off, shp in first.layout}
    lr = SG.learning_rate(STEP_LR0, 1, 1, True)
    zeros = {k: np.zeros(np.shape(v)) for k, v in before.items()}
    want, _, _, norm, _ = SG.train_step(before, raw, zeros, zeros, 1, lr, hp.adam_beta1, hp.adam_beta2)
    assert norm > 1.0, norm
    after = first.variables()
    bn = lambda k: k.endswith("batch_normalization")
    worst = max((float(np.abs(after[k][:2].astype(np.float64) - want[k][:2]).max()) if bn(k) else float(np.abs(after[k].astype(np.float64) - want[k]).max()), k)
                for k in want)
    print("training=%s: gradient norm %.4f, worst |variable - checker| %.3e (%s), bar %.3e" % (training, norm, worst[0], worst[1], STEP_ATOL * lr / 1e-3))
    assert worst[0] <= STEP_ATOL * (lr / 1e-3), worst
    at = first._stats_at
    if training:
        assert own[at:].any() and first_mismatch(own[at:], other[at:]) is not None
        assert first_mismatch(own[at:], np.concatenate([s.cpu().numpy() for s in alone._stats])) is None
        stats, off, worst_m = {}, at, 0.0
        for which, count in zip(("encoder", "post"), first._stat_floats):
            stats.update({k: v.numpy() for k, v in first.model._split_stats(__import__("torch").from_numpy(mean[off:off + count]), which).items()})
            off += count
        assert off == mean.size and len(stats) == sum(1 for k in after if bn(k))
        for k, s in stats.items():
            mv = TM.moving_average(before[k][2:], s)
            worst_m = max(worst_m, float(np.abs(after[k][2:] - mv).max()) / float(np.abs(mv).max()))
            assert (after[k][2:] != before[k][2:]).any(), k
        print("moving statistics against the float64 formula at the mean statistics: worst %.3e of a tensor's maximum" % worst_m)
        assert worst_m <= 1e-6, worst_m
    else:
        assert not own[at:].any()
        assert all(first_mismatch(after[k][2:], before[k][2:]) is None for k in after if bn(k))

    # a peer that failed: its zeros and its flag arrive, and nothing moves, bit for bit
    def failed_peer(flat, group):
        flat[n] += 1.0
        return 2
    stuck = _trainer(training, hp, h.w, allreduce=failed_peer)
    blob = stuck.model._blob.clone()
    assert stuck.step(*batch_a)["loss"] == out["loss"]
    assert stuck.peer_failure() and stuck.global_step == 0
    same_outputs(before, stuck.variables(), "a step whose reduction carries a failed rank")
    assert first_mismatch(stuck.model._blob.cpu().numpy(), blob.cpu().numpy()) is None and not stuck.m.any() and not stuck.v.any()
    # this rank failing: it joins with zeros and the flag set, and applies nothing
    def see(flat, group):
        box["failed"] = flat.clone()
        return 2
    gone = _trainer(training, hp, h.w, allreduce=see)
    assert gone.step(None, None, None, None, None, failed=True) is None and gone.global_step == 0 and gone.peer_failure()
    sent = box["failed"].cpu().numpy()
    assert sent[n] == 1.0 and not np.delete(sent, n).any()
    same_outputs(before, gone.variables(), "a failed rank")
    # and a rank whose step raises joins the same way before it re-raises
    with pytest.raises(Exception):
        gone.step(batch_a[0], batch_a[1], batch_a[2], batch_a[3][:, :3], batch_a[4], batch_a[5])
    sent = box["failed"].cpu().numpy()
    assert sent[n] == 1.0 and not np.delete(sent, n).any() and gone.global_step == 0


# ---------------------------------------------------------------- the command
def _run(argv, hp):
    from twvk_amd import train_tacotron
    lines = []
    out = train_tacotron.main(argv, hp=hp, log=lines.append)
    return out, lines


def test_train_tacotron_command(tmp_path):
    from scipy.io import wavfile
    from twvk_amd.synthesizer import Synthesizer
    hp = _hp()
    dirs = write_directories(tmp_path / "data", hp, speakers=2, per_speaker=12, seed=3, frames=(6, 34), tokens=(3, 12))
    common = ["--data_paths", ",".join(dirs), "--batch_size", "3", "--random_seed", "7", "--summary_interval", "2", "--test_interval", "3",
              "--checkpoint_interval", "3"]
    out, lines = _run(["--log_dir", str(tmp_path / "logs")] + common + ["--num_steps", "6"], hp)
    d = out["model_dir"]
    assert out["step"] == 6 and len(out["losses"]) == 6 and np.isfinite(out["losses"]).all()
    assert os.path.dirname(d) == str(tmp_path / "logs") and os.path.basename(d).startswith("speaker_0+speaker_1_")
    assert sum(1 for l in lines if l.startswith("Step ")) == 6 and any(l.startswith("Step 6 ") for l in lines)
    for step in (3, 6):
        assert os.path.exists(os.path.join(d, "model.ckpt-%d.index" % step)) and os.path.exists(os.path.join(d, "model.ckpt-%d.data-00000-of-00001" % step))
    params = json.load(open(os.path.join(d, "params.json"), encoding="utf-8"))
    assert params["num_speakers"] == 2 and params["num_freq"] == 129
    # the outputs of step 3: one train example, the four test examples
    r = hp.reduction_factor
    for prefix, count in (("train", 1), ("test", 4)):
        for idx in range(count):
            base = os.path.join(d, "%s-step-%09d" % (prefix, 3))
            sr, wav = wavfile.read("%s-audio%03d.wav" % (base, idx))
            al = np.load("%s-align%03d.npy" % (base, idx))
            assert sr == hp.sample_rate and wav.dtype == np.int16 and al.ndim == 2 and 1 <= al.shape[1] <= MAX_ITERS and 3 <= al.shape[0] <= 12
            assert wav.shape == (hp.hop_size * (al.shape[1] * r - 1),) and np.isfinite(al).all()
        assert not os.path.exists("%s-audio%03d.wav" % (base, count))
    assert os.path.exists(os.path.join(d, "test-step-%09d-audio003.wav" % 6))
    stats = [json.loads(l) for l in open(os.path.join(d, "stats.jsonl"))]
    assert [s["step"] for s in stats] == [2, 4, 6]
    for s in stats:
        assert s["learning_rate"] > 0 and np.isfinite([s["train"]["loss"], s["test"]["loss"], s["gap_test-train"]["loss_without_coeff"]]).all()
        assert s["gap_test-train"]["mel_loss"] == pytest.approx(s["test"]["mel_loss"] - s["train"]["mel_loss"])
    # Synthesizer.load reads the run's last checkpoint
    s = Synthesizer()
    s.load(d, num_speakers=2, hparams=_hp())
    got = s.infer([[5, 6, 7, 1]], [1])
    assert np.isfinite(got["mel"].cpu().numpy()).all()
    last = out["trainer"].variables()
    # the same seed: the same bytes in model.ckpt-6
    out2, _ = _run(["--log_dir", str(tmp_path / "logs2")] + common + ["--num_steps", "6"], _hp())
    assert out2["losses"] == out["losses"]
    for suffix in (".index", ".data-00000-of-00001"):
        a, b = (open(os.path.join(x["model_dir"], "model.ckpt-6" + suffix), "rb").read() for x in (out, out2))
        assert a == b, suffix
    # --load_path continues at step 7
    out3, lines3 = _run(["--load_path", d] + common + ["--num_steps", "8"], _hp())
    assert out3["model_dir"] == d and out3["step"] == 8 and len(out3["losses"]) == 2
    assert [l.split()[1] for l in lines3 if l.startswith("Step ")] == ["7", "8"]
    # --initialize_path: the restored weights, the step from 0
    out4, _ = _run(["--log_dir", str(tmp_path / "logs4"), "--initialize_path", out2["model_dir"]] + common + ["--num_steps", "0"], _hp())
    assert out4["step"] == 0 and out4["model_dir"] != out2["model_dir"] and not out4["trainer"].randomly_initialized
    same_outputs(last, out4["trainer"].variables(), "variables restored by --initialize_path")
    out5, lines5 = _run(["--log_dir", str(tmp_path / "logs5"), "--initialize_path", out2["model_dir"]] + common + ["--num_steps", "1"], _hp())
    assert out5["step"] == 1 and [l.split()[1] for l in lines5 if l.startswith("Step ")] == ["1"]


def test_twenty_steps_from_the_initial_values_lower_the_loss():
    """one fixed batch (C-length-one's) at tacotron_initial_learning_rate 1e-3, mode 1: the rate of the existing twenty-step test"""
    from twvk_amd.tacotron import Tacotron
    from twvk_amd.tacotron_train import TacotronTrainer, initial_tensors
    h = whole_case("C-length-one")
    hp = hparams(max_iters=8, **dict(SMALL, tacotron_initial_learning_rate=TWENTY_LR0, decay_learning_rate_mode=TWENTY_MODE))
    t = TacotronTrainer(Tacotron(hp, num_speakers=h.speakers), randomly_initialized=False)
    tensors = t.init_weights(seed=11)
    same_outputs(initial_tensors(t.model.specs, hp, 11), t.variables(), "init_weights")
    assert t.global_step == 0 and sorted(tensors) == sorted(n for n, _ in t.model.specs)
    batch = (h.tok, h.ln, h.spk, h.tgt, h.lin_tgt, h.coeff)
    losses = [t.step(*batch)["loss"] for _ in range(TWENTY_STEPS)]
    losses.append(t.step(*batch)["loss"])
    print("losses:", " ".join("%.5f" % x for x in losses))
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses


# ---------------------------------------------------------------- two ranks on two GPUs
def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_on_two_gpus(tmp_path):
    """a four-step train_tacotron on two ranks under torch.distributed.run (the launcher bench.py --gpus 2 uses; tests/tacotron_two_ranks.py is
    one rank): both ranks' final variables() digests are equal -- the all-reduced gradient and the mean batch statistics keep the replicas
    identical although each rank read its own share of the examples -- and they differ from a one-rank run's over the same directories."""
    import subprocess
    import sys
    import torch
    if (torch.cuda.device_count() if torch.cuda.is_available() else 0) < 2:
        pytest.skip("needs >= 2 visible GPUs (the driver's multi-GPU node)")
    here = os.path.dirname(os.path.abspath(__file__))
    driver = os.path.join(here, "tacotron_two_ranks.py")
    dirs = write_directories(tmp_path / "data", _hp(), speakers=2, per_speaker=16, seed=3, frames=(6, 34), tokens=(3, 12))
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

    def launch(cmd, tag):
        r = subprocess.run(cmd + [str(tmp_path / ("logs_" + tag)), str(tmp_path / tag), ",".join(dirs)], cwd=os.path.dirname(here), env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    launch([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
            "--master-port", str(_free_port()), driver], "two")
    launch([sys.executable, driver], "one")
    two = [json.load(open(str(tmp_path / ("two.rank%d.json" % k)))) for k in range(2)]
    one = json.load(open(str(tmp_path / "one.rank0.json")))
    assert [t["rank"] for t in two] == [0, 1] and all(t["world"] == 2 and t["step"] == 4 and not t["peer_failure"] for t in two) and one["world"] == 1
    assert all(np.isfinite(t["losses"]).all() and len(t["losses"]) == 4 for t in two + [one])
    assert two[0]["model_dir"] == two[1]["model_dir"]                     # rank 0 decided the directory, once
    assert two[0]["losses"] != two[1]["losses"]                           # each rank on its own share of the examples
    assert two[0]["digest"] == two[1]["digest"]
    assert one["digest"] != two[0]["digest"] and one["step"] == 4
