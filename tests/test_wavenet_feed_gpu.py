"""The WaveNet feed on the device: twv_wavenet_crop_stage against numpy slicing bit for bit into outputs that sit inside
NaN-filled tensors, DeviceFeederWavenet against DataFeederWavenet over three refills and through WaveNetTrainer.step, and
train_vocoder.main under the three settings of TWV_VOCODER_CORPUS."""
import os

import numpy as np
import pytest

from wavenet_feed_cases import RECEPTIVE_FIELD, SCHEDULE_COUNTS, batches_to_cross, feed_hp, same_bits, write_corpus

pytestmark = pytest.mark.gpu
GUARD = 4                    # floats: the outputs must start on a 16-byte boundary


# ---------------------------------------------------------------- the kernel
def _pools(hop, M, counts, seed):
    """examples of the given frame counts packed as CorpusIndex packs them: (audio pool, mel pool, table); the pools end where the last
    example ends"""
    from twvk_amd.wavenet_feed import ROW_DTYPE
    rng = np.random.RandomState(seed)
    audio, mel, rows = [], [], []
    a_at = m_at = 0
    for i, n in enumerate(counts):
        pad = -a_at % 4
        audio.append(np.full(pad, np.nan, np.float32))             # (the words between two examples are never read: NaN would show)
        a_at += pad
        rows.append((a_at, m_at, n, i % 3))
        audio.append(rng.uniform(-1, 1, n * hop).astype(np.float32))
        mel.append(rng.uniform(-4, 4, n * M).astype(np.float32))
        a_at += n * hop
        m_at += n * M
    return np.concatenate(audio), np.concatenate(mel), np.array(rows, ROW_DTYPE)


GEOMETRIES = [(1, 1, 1, 1), (3, 4, 2, 3), (4, 4, 1, 3), (5, 3, 7, 5), (300, 80, 26, 8), (300, 80, 26, 64)]


@pytest.mark.parametrize("hop, M, F, B", GEOMETRIES)
def test_crop_kernel_equals_numpy_slicing_bit_for_bit(hop, M, F, B):
    """the picks: the first example at start 0; the last example of the pool cropped to its last frame (the pool ends exactly where the
    crop does); that example again at start 1 (the same example twice; with an odd hop a source that starts off the 16-byte grid); the
    rest drawn.  Where B is smaller than that list it takes several calls, each into its own NaN-filled tensors."""
    import torch
    from twvk_amd.wavenet_feed import crop_stage
    counts = [F + 2, F, 2 * F + 3, F + 1, F + 5]
    audio_pool, mel_pool, table = _pools(hop, M, counts, seed=hop + M + F + B)
    last = len(counts) - 1
    assert table["audio_offset"][last] + counts[last] * hop == audio_pool.size and table["mel_offset"][last] + counts[last] * M == mel_pool.size
    rng = np.random.RandomState(B)
    picks = [(0, 0), (last, counts[last] - F), (last, 1)]
    while len(picks) < B or len(picks) % B:
        ex = int(rng.randint(len(counts)))
        picks.append((ex, int(rng.randint(counts[ex] - F + 1))))
    picks = np.asarray(picks, np.int32)
    if hop % 2:
        assert any((table["audio_offset"][e] + s * hop) % 4 for e, s in picks), "no crop starts off the 16-byte grid"
    dev = "cuda:0"
    a_dev, m_dev = torch.from_numpy(audio_pool).to(dev), torch.from_numpy(mel_pool).to(dev)
    t_dev = torch.from_numpy(table.view(np.int32).copy()).to(dev)
    for at in range(0, len(picks), B):
        pk = np.ascontiguousarray(picks[at:at + B])
        na, nl = B * F * hop, B * F * M
        big_a = torch.full((GUARD + na + GUARD + 3,), float("nan"), device=dev)
        big_l = torch.full((GUARD + nl + GUARD + 3,), float("nan"), device=dev)
        big_g = torch.full((GUARD + B + GUARD,), -1, dtype=torch.int32, device=dev)
        out = (big_a[GUARD:GUARD + na].view(B, F * hop), big_l[GUARD:GUARD + nl].view(B, F, M), big_g[GUARD:GUARD + B])
        crop_stage(a_dev, m_dev, table, t_dev, pk, torch.from_numpy(pk).to(dev), F, hop, M, out=out)
        torch.cuda.synchronize()
        want_a = np.stack([audio_pool[table["audio_offset"][e] + s * hop:table["audio_offset"][e] + (s + F) * hop] for e, s in pk])
        want_l = np.stack([mel_pool[table["mel_offset"][e] + s * M:table["mel_offset"][e] + (s + F) * M].reshape(F, M) for e, s in pk])
        assert not np.isnan(want_a).any() and want_a.shape == (B, F * hop) and want_l.shape == (B, F, M)
        got_a, got_l, got_g = big_a.cpu().numpy(), big_l.cpu().numpy(), big_g.cpu().numpy()
        assert same_bits(got_a[GUARD:GUARD + na].reshape(B, F * hop), want_a), ("audio", at)
        assert same_bits(got_l[GUARD:GUARD + nl].reshape(B, F, M), want_l), ("local_condition", at)
        assert np.array_equal(got_g[GUARD:GUARD + B], table["speaker_id"][pk[:, 0]]), ("gc_ids", at)
        for name, got, n in (("audio", got_a, na), ("local_condition", got_l, nl)):
            assert np.isnan(got[:GUARD]).all() and np.isnan(got[GUARD + n:]).all(), (name, "guard words", at)
        assert (got_g[:GUARD] == -1).all() and (got_g[GUARD + B:] == -1).all(), ("gc_ids", "guard words", at)


def test_crop_stage_refuses_a_crop_past_its_example_on_device_pointers():
    import torch
    from twvk_amd._lib import TwvError
    from twvk_amd.wavenet_feed import crop_stage
    audio_pool, mel_pool, table = _pools(5, 3, [4, 6], seed=0)
    dev = "cuda:0"
    pk = np.array([[0, 0], [1, 5]], np.int32)
    with pytest.raises(TwvError, match="twv_amd error 1: pick 1: frames 5 .. 7 outside the 6 frames of example 1"):
        crop_stage(torch.from_numpy(audio_pool).to(dev), torch.from_numpy(mel_pool).to(dev), table, torch.from_numpy(table.view(np.int32).copy()).to(dev),
                   pk, torch.from_numpy(pk).to(dev), 2, 5, 3)


# ---------------------------------------------------------------- the feeder
def test_device_feeder_equals_the_host_feeder_over_three_refills(tmp_path):
    from twvk_amd.train_vocoder import DataFeederWavenet
    from twvk_amd.wavenet_feed import CorpusIndex, DeviceFeederWavenet
    hp = feed_hp()
    dirs = write_corpus(tmp_path, hp, SCHEDULE_COUNTS)
    n = batches_to_cross(hp.wavenet_batch_size)
    for rank, world in ((0, 1), (1, 2)):
        host = DataFeederWavenet(dirs, hp.wavenet_batch_size, RECEPTIVE_FIELD, gc_enable=True, hp=hp, rank=rank, world=world)
        np.random.seed(11)
        want = [host.next_batch() for _ in range(n)]
        feeder = DeviceFeederWavenet(CorpusIndex(dirs, hp.wavenet_batch_size, RECEPTIVE_FIELD, gc_enable=True, hp=hp, rank=rank, world=world), "cuda:0")
        np.random.seed(11)
        got = [feeder.next_batch() for _ in range(n)]              # (all in flight at once: the pinned slots of the picks alternate)
        for k in range(n):
            assert all(t.is_cuda for t in got[k])
            for name, g, w in zip(("audio", "local_condition", "gc_ids"), got[k], want[k]):
                assert same_bits(g.cpu().numpy(), w), (rank, world, k, name)


def test_both_feeders_train_the_same_losses(tmp_path):
    """the batches of both routes through WaveNetTrainer.step on a two-layer model: the losses are the same bits.  The training step is
    built for num_mels = 80 and asks for more samples than the receptive field (35 here), so this corpus has 80 mels at hop 32 (the
    model's upsample_factor (2, 4, 4)) and crops of 4 frames; the schedule test's corpus (4 mels, hop 5) is the test above."""
    import torch
    from train_cases import _model, case_data
    from twvk_amd.train import WaveNetTrainer
    from twvk_amd.train_vocoder import DataFeederWavenet
    from twvk_amd.wavenet_feed import CorpusIndex, DeviceFeederWavenet
    B, dil, up = 3, [1, 2], (2, 4, 4)
    hp = feed_hp(hop_size=32, num_mels=80, frames=4, batch=B, extra=7)
    dirs = write_corpus(tmp_path, hp, ((5, 12, 4, 9, 7), (6, 4, 11, 5, 8)), seed=3)
    tensors = case_data(dil=dil, B=B, Tm=4, up=up)[0]
    kw = dict(B=B, dil=dil, S=64, use_bias=True, up=up, out_channels=30, ifw=32, G=32, gc_card=2, scalar_input=True, Q=256, device="cuda:0")
    n = batches_to_cross(B)
    losses = {}
    for route in ("host", "device"):
        tr = WaveNetTrainer(_model(**kw), sample_size=hp.sample_size)
        assert tr.sample_size == 128
        tr.load_weights(tensors)
        if route == "host":
            feeder = DataFeederWavenet(dirs, B, RECEPTIVE_FIELD, gc_enable=True, hp=hp)
        else:
            feeder = DeviceFeederWavenet(CorpusIndex(dirs, B, RECEPTIVE_FIELD, gc_enable=True, hp=hp), "cuda:0")
        np.random.seed(21)
        kept = []
        for _ in range(n):
            kept.append(tr.step(*feeder.next_batch()).clone())
        losses[route] = torch.stack(kept).cpu().numpy()
    assert np.isfinite(losses["host"]).all() and len(set(losses["host"].ravel().tolist())) > n // 2
    assert same_bits(losses["host"], losses["device"])


# ---------------------------------------------------------------- the command
def test_train_vocoder_is_the_same_run_on_every_route(tmp_path, monkeypatch):
    """train_vocoder.main for 6 steps on a tiny corpus at the default hop and mel count, under TWV_VOCODER_CORPUS = host, device and
    unset: the routes' names, the logged losses and every variable of model.ckpt-6"""
    from twvk_amd import checkpoint as ckpt
    from twvk_amd.hparams import hparams
    from twvk_amd.train_vocoder import main as tv_main
    saved = {k: getattr(hparams, k) for k in ("dilations", "wavenet_batch_size", "sample_size", "skip_channels")}
    try:
        hparams.dilations = [1, 2, 4, 8, 1, 2, 4, 8]; hparams.wavenet_batch_size = 2; hparams.sample_size = 1200
        hparams.skip_channels = 64
        dirs = write_corpus(tmp_path / "data", hparams, ((5, 9, 4, 7), (6, 3, 8)), seed=5)
        monkeypatch.delenv("TWV_VOCODER_CORPUS_GB", raising=False)
        runs = {}
        for setting in ("host", "device", None):
            if setting is None:
                monkeypatch.delenv("TWV_VOCODER_CORPUS", raising=False)
            else:
                monkeypatch.setenv("TWV_VOCODER_CORPUS", setting)
            logdir = str(tmp_path / ("run_%s" % setting))
            lines = []
            r = tv_main(["--data_dir", ",".join(dirs), "--logdir", logdir, "--checkpoint_every", "6", "--num_steps", "6"], log=lines.append)
            assert r["step"] == 6 and np.isfinite(r["loss"])
            steps = [l.split(", (")[0] for l in lines if l.startswith("step ")]
            assert len(steps) == 6
            runs[setting] = (r["feeder"], steps, r["loss"], ckpt.read_bundle(os.path.join(logdir, "model.ckpt-6"), verify=True))
        assert [runs[s][0] for s in ("host", "device", None)] == ["host", "device", "device"]
        want = runs["host"]
        assert len(set(want[1])) == 6
        for setting in ("device", None):
            got = runs[setting]
            assert got[1] == want[1] and got[2] == want[2], setting
            assert sorted(got[3]) == sorted(want[3])
            for name in want[3]:
                assert same_bits(np.asarray(got[3][name]), np.asarray(want[3][name])), (setting, name)
    finally:
        for k, v in saved.items():
            setattr(hparams, k, v)
