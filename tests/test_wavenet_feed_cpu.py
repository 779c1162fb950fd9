"""The WaveNet feed on the host: the C surface of twv_wavenet_crop_stage and its refusals on host addresses,
CorpusIndex's schedule against DataFeederWavenet bit for bit, the pack's refusals, the prefetch thread, and the route rule of
train_vocoder.choose_feeder.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import twvk_amd  # noqa: F401
from wavenet_feed_cases import RECEPTIVE_FIELD, SCHEDULE_COUNTS, assert_same_batch, batches_to_cross, feed_hp, write_corpus


# ---------------------------------------------------------------- the C surface
def test_symbol_is_exported_declared_and_bound():
    from twvk_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "twv_amd.h")).read()
    L = _lib.lib()
    nm = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    name = "twv_wavenet_crop_stage"
    assert name in _lib.EXPORTS and name + "(" in header and "twv_wavenet_feed_row" in header
    assert (" T " + name + "\n") in nm
    assert getattr(L, name).argtypes is not None and len(getattr(L, name).argtypes) == 17
    assert "wf_crop_kernel" in nm, "the gfx950 kernel wf_crop_kernel must be in the library"
    from twvk_amd.wavenet_feed import ROW_DTYPE
    assert ROW_DTYPE.itemsize == 24 and [ROW_DTYPE.fields[k][1] for k in ("audio_offset", "mel_offset", "n_frames", "speaker_id")] == [0, 8, 16, 20]


def test_crop_stage_refuses_on_the_host():
    """every refusal of twv_wavenet_crop_stage is decided from the host's table and picks before anything is launched: host addresses
    suffice for every pointer, and each refusal is `twv_amd error 1` (TWV_E_INVALID)"""
    from twvk_amd import _lib
    from twvk_amd.wavenet_feed import ROW_DTYPE
    L = _lib.lib()
    hop, M, F = 5, 4, 2
    # two examples of 3 and 4 frames: audio at 0 and 16 (rounded up from 15), mels at 0 and 12; the pools end where example 1 ends
    table = np.array([(0, 0, 3, 0), (16, 12, 4, 1)], ROW_DTYPE)
    audio_floats, mel_floats = 16 + 4 * hop, 12 + 4 * M
    picks = np.array([[0, 0], [1, 2]], np.int32)
    raw = np.zeros(256 + 4, np.float32)
    o = raw.ctypes.data + (-raw.ctypes.data) % 16                                              # a 16-byte aligned host address
    p = C.c_void_p(o)
    names = ("audio_pool", "mel_pool", "table_host", "table_dev", "picks_host", "picks_dev", "audio", "local_condition", "gc_ids")

    def call(tab=table, pk=picks, n_examples=2, batch=2, frames=F, hop_size=hop, num_mels=M, audio_floats=audio_floats, mel_floats=mel_floats,
             **ptr):
        a = {k: p for k in names}
        a["table_host"], a["picks_host"] = tab.ctypes.data_as(C.c_void_p), pk.ctypes.data_as(C.c_void_p)
        a.update(ptr)
        rc = L.twv_wavenet_crop_stage(a["audio_pool"], audio_floats, a["mel_pool"], mel_floats, a["table_host"], a["table_dev"], n_examples,
                                      a["picks_host"], a["picks_dev"], batch, frames, hop_size, num_mels, a["audio"], a["local_condition"], a["gc_ids"],
                                      None)
        if rc:
            with pytest.raises(_lib.TwvError, match="twv_amd error 1"):
                _lib.check(rc)
        return rc, L.twv_last_error().decode()
    for k in names:
        assert call(**{k: None}) == (1, "null argument"), k
    assert call(batch=0)[0] == 1 and call(frames=0)[0] == 1 and call(hop_size=0)[0] == 1 and call(num_mels=0)[0] == 1 and call(n_examples=0)[0] == 1
    rc, words = call(pk=np.array([[0, 0], [2, 0]], np.int32))
    assert rc == 1 and "pick 1" in words and "example 2 outside [0, 2)" in words
    assert call(pk=np.array([[-1, 0], [1, 0]], np.int32))[0] == 1
    rc, words = call(pk=np.array([[0, 2], [1, 2]], np.int32))                                  # start + frames = n_frames + 1
    assert rc == 1 and "pick 0" in words and "frames 2 .. 4 outside the 3 frames" in words
    assert call(pk=np.array([[0, 1], [1, -1]], np.int32))[0] == 1
    for which, floats in (("audio_floats", audio_floats - 1), ("mel_floats", mel_floats - 1)):  # row 1 reaches one float past a pool
        rc, words = call(**{which: floats})
        assert rc == 1 and "pick 1" in words and "leaves its pool" in words, which
    bad = table.copy()
    bad["audio_offset"][0] = -4
    assert call(tab=bad)[0] == 1
    for k in ("audio", "local_condition"):
        rc, words = call(**{k: C.c_void_p(o + 4)})
        assert rc == 1 and "16-byte aligned" in words, k


# ---------------------------------------------------------------- the schedule
def _numpy_batch(index, picks):
    """the picks applied to the packed arrays by plain numpy slicing"""
    example, start, speaker = picks
    hop, F, M = index.hop_size, index.max_frames, index.num_mels
    audio, lc = [], []
    for ex, s in zip(example, start):
        row = index.table[ex]
        a = index.audio_pool[row["audio_offset"]:row["audio_offset"] + row["n_frames"] * hop]
        m = index.mel_pool[row["mel_offset"]:row["mel_offset"] + row["n_frames"] * M].reshape(row["n_frames"], M)
        audio.append(a[s * hop:(s + F) * hop])
        lc.append(m[s:s + F])
    assert all(index.table["speaker_id"][ex] == spk for ex, spk in zip(example, speaker))
    return np.stack(audio), np.stack(lc), speaker


@pytest.mark.parametrize("rank,world", [(0, 1), (0, 2), (1, 2)])
def test_schedule_equals_the_host_feeder(tmp_path, rank, world):
    """over three refills -- the offsets wrap and the lists are reshuffled many times (7 files, 48 examples per directory and refill),
    the too-short file of each directory is skipped and consumes its offset -- the index's picks cut the host feeder's batches"""
    from twvk_amd.train_vocoder import DataFeederWavenet
    from twvk_amd.wavenet_feed import CorpusIndex
    hp = feed_hp()
    dirs = write_corpus(tmp_path, hp, SCHEDULE_COUNTS)
    host = DataFeederWavenet(dirs, hp.wavenet_batch_size, RECEPTIVE_FIELD, gc_enable=True, hp=hp, rank=rank, world=world)
    index = CorpusIndex(dirs, hp.wavenet_batch_size, RECEPTIVE_FIELD, gc_enable=True, hp=hp, rank=rank, world=world)
    assert (index.sample_size, index.max_frames) == (host.sample_size, host.max_frames) == (20, 4)
    assert index.n_examples == sum(len(p) for p in host.path_dict.values()) == {(0, 1): 14, (0, 2): 8, (1, 2): 6}[rank, world]
    assert all(o % 4 == 0 for o in index.table["audio_offset"]) and index.packed_bytes == 4 * (index.audio_pool.size + index.mel_pool.size)
    assert np.array_equal(np.diff(index.table["mel_offset"]), index.table["n_frames"][:-1] * hp.num_mels)      # packed densely
    n = batches_to_cross(hp.wavenet_batch_size)
    np.random.seed(7 + rank)
    want = [host.next_batch() for _ in range(n)]
    np.random.seed(7 + rank)
    starts = set()
    for k in range(n):
        picks = index.next_picks()
        assert all(a.dtype == np.int32 and a.shape == (hp.wavenet_batch_size,) for a in picks)
        assert_same_batch(_numpy_batch(index, picks), want[k], "batch %d" % k)
        starts.update(picks[1].tolist())
        assert not any(index.table["n_frames"][e] == 4 for e in picks[0])
    assert len(starts) > 8
    assert want[0][0].shape == (3, 20) and want[0][1].shape == (3, 4, 4) and {int(g) for b in want for g in b[2]} == {0, 1}


def test_a_directory_with_fewer_files_than_ranks_is_shared_whole(tmp_path):
    from twvk_amd.train_vocoder import DataFeederWavenet
    from twvk_amd.wavenet_feed import CorpusIndex
    hp = feed_hp()
    dirs = write_corpus(tmp_path, hp, ((9, 14), (6, 4, 11, 30, 8, 7, 19)))
    for rank in range(3):
        host = DataFeederWavenet(dirs, hp.wavenet_batch_size, RECEPTIVE_FIELD, hp=hp, rank=rank, world=3)
        index = CorpusIndex(dirs, hp.wavenet_batch_size, RECEPTIVE_FIELD, hp=hp, rank=rank, world=3)
        assert [os.path.basename(index.names[e]) for e in index.path_dict[dirs[0]]] == host.path_dict[dirs[0]] == ["utt00.npz", "utt01.npz"]
        assert [os.path.basename(index.names[e]) for e in index.path_dict[dirs[1]]] == host.path_dict[dirs[1]]
        assert len(index.path_dict[dirs[1]]) == (3 if rank == 0 else 2)
        np.random.seed(rank)
        want = [host.next_batch() for _ in range(40)]
        np.random.seed(rank)
        for k in range(40):
            assert_same_batch(_numpy_batch(index, index.next_picks()), want[k], "rank %d batch %d" % (rank, k))


def test_pack_refusals(tmp_path):
    from twvk_amd.wavenet_feed import CorpusIndex, CorpusTooLarge
    hp = feed_hp()
    dirs = write_corpus(tmp_path / "ok", hp, ((9, 14), (6, 11)))
    rng = np.random.RandomState(1)
    np.savez(os.path.join(dirs[1], "utt07_bad.npz"), audio=rng.rand(7 * hp.hop_size + 1).astype(np.float32), mel=rng.rand(7, hp.num_mels).astype(np.float32))
    with pytest.raises(ValueError, match="utt07_bad.npz"):
        CorpusIndex(dirs, 3, RECEPTIVE_FIELD, hp=hp)
    np.savez(os.path.join(dirs[1], "utt07_bad.npz"), audio=rng.rand(14 * hp.hop_size).astype(np.float32), mel=rng.rand(7, hp.num_mels).astype(np.float32))
    with pytest.raises(ValueError, match="utt07_bad.npz"):                                # a whole multiple, but not hop_size
        CorpusIndex(dirs, 3, RECEPTIVE_FIELD, hp=hp)
    os.remove(os.path.join(dirs[1], "utt07_bad.npz"))
    assert CorpusIndex(dirs, 3, RECEPTIVE_FIELD, hp=hp).n_examples == 4
    (tmp_path / "empty").mkdir()
    with pytest.raises(ValueError, match="no .npz examples in"):
        CorpusIndex([dirs[0], str(tmp_path / "empty")], 3, RECEPTIVE_FIELD, hp=hp)
    with pytest.raises(CorpusTooLarge, match="after 2 of 4 examples"):
        CorpusIndex(dirs, 3, RECEPTIVE_FIELD, hp=hp, max_bytes=4 * (9 * 5 + 3 + 9 * 4 + 14 * 5 + 14 * 4) - 1)
    # a directory whose every example is too short: the host feeder's error, when the first batch is asked for
    short = write_corpus(tmp_path / "short", hp, ((3, 4),))
    with pytest.raises(ValueError, match="no example in .* is longer than 20 samples"):
        CorpusIndex(short, 3, RECEPTIVE_FIELD, hp=hp).next_picks()


# ---------------------------------------------------------------- the prefetch thread
def test_prefetch_feeder_gives_the_same_batches_in_order(tmp_path):
    import threading
    from twvk_amd.train_vocoder import DataFeederWavenet
    from twvk_amd.wavenet_feed import PrefetchFeeder
    hp = feed_hp()
    dirs = write_corpus(tmp_path, hp, SCHEDULE_COUNTS)
    n = batches_to_cross(hp.wavenet_batch_size)
    np.random.seed(3)
    plain = DataFeederWavenet(dirs, hp.wavenet_batch_size, RECEPTIVE_FIELD, hp=hp)
    want = [plain.next_batch() for _ in range(n)]
    before = threading.active_count()
    feeder = PrefetchFeeder(DataFeederWavenet(dirs, hp.wavenet_batch_size, RECEPTIVE_FIELD, hp=hp))
    np.random.seed(3)                                            # (before the first next_batch: the thread starts there)
    for k in range(n):
        assert_same_batch(feeder.next_batch(), want[k], "batch %d" % k)
    feeder.close()
    assert threading.active_count() == before
    with pytest.raises(RuntimeError, match="closed"):
        feeder.next_batch()


def test_prefetch_feeder_raises_where_the_batch_was_due():
    from twvk_amd.wavenet_feed import PrefetchFeeder

    class Failing(object):
        def __init__(self, fail_at):
            self.k, self.fail_at = 0, fail_at

        def next_batch(self):
            self.k += 1
            if self.k == self.fail_at:
                raise KeyError("batch %d" % self.k)
            return self.k
    for fail_at in (1, 2, 5):
        feeder = PrefetchFeeder(Failing(fail_at))
        assert [feeder.next_batch() for _ in range(fail_at - 1)] == list(range(1, fail_at))
        for _ in range(2):                                       # the call that was due the batch, and every later one
            with pytest.raises(KeyError, match="batch %d" % fail_at):
                feeder.next_batch()
        feeder.close()


# ---------------------------------------------------------------- the route rule
@pytest.fixture
def route_env(tmp_path, monkeypatch):
    from twvk_amd import train_vocoder
    hp = feed_hp()
    dirs = write_corpus(tmp_path, hp, SCHEDULE_COUNTS)
    queried = []
    monkeypatch.setattr(train_vocoder, "free_device_bytes", lambda device: queried.append(device) or (1 << 30))
    monkeypatch.delenv("TWV_VOCODER_CORPUS", raising=False)
    monkeypatch.delenv("TWV_VOCODER_CORPUS_GB", raising=False)
    return train_vocoder, hp, dirs, queried, monkeypatch


def _choose(train_vocoder, hp, dirs, lines):
    return train_vocoder.choose_feeder(dirs, hp, RECEPTIVE_FIELD, True, 0, 1, "cuda:0", lines.append)


def test_auto_above_the_cap_feeds_from_the_host_behind_the_thread(route_env):
    from twvk_amd.wavenet_feed import PrefetchFeeder
    train_vocoder, hp, dirs, queried, monkeypatch = route_env
    monkeypatch.setenv("TWV_VOCODER_CORPUS_GB", "1e-6")          # 1000 bytes
    lines = []
    reader, route = _choose(train_vocoder, hp, dirs, lines)
    assert route == "host+prefetch" and isinstance(reader, PrefetchFeeder) and isinstance(reader.feeder, train_vocoder.DataFeederWavenet)
    assert len(lines) == 1 and "does not fit" in lines[0] and "14 examples" in lines[0] and "limit 1000 bytes" in lines[0] and queried == ["cuda:0"]
    # half of the free memory is a cap of its own
    monkeypatch.delenv("TWV_VOCODER_CORPUS_GB")
    monkeypatch.setattr(train_vocoder, "free_device_bytes", lambda device: 4000)
    lines = []
    reader, route = _choose(train_vocoder, hp, dirs, lines)
    assert route == "host+prefetch" and "limit 2000 bytes" in lines[0]
    # and what it feeds is the host feeder's batches
    np.random.seed(5)
    plain = train_vocoder.DataFeederWavenet(dirs, hp.wavenet_batch_size, RECEPTIVE_FIELD, gc_enable=True, hp=hp)
    want = [plain.next_batch() for _ in range(4)]
    np.random.seed(5)
    for k in range(4):
        assert_same_batch(reader.next_batch(), want[k], "batch %d" % k)
    reader.close()


def test_auto_with_a_pack_that_raises_feeds_from_the_host_and_device_raises(route_env):
    train_vocoder, hp, dirs, queried, monkeypatch = route_env
    rng = np.random.RandomState(2)
    np.savez(os.path.join(dirs[0], "utt99_bad.npz"), audio=rng.rand(33).astype(np.float32), mel=rng.rand(6, hp.num_mels).astype(np.float32))
    lines = []
    reader, route = _choose(train_vocoder, hp, dirs, lines)
    assert route == "host+prefetch" and len(lines) == 1 and "utt99_bad.npz" in lines[0] and "15 examples" in lines[0]
    monkeypatch.setenv("TWV_VOCODER_CORPUS", "device")
    with pytest.raises(ValueError, match="utt99_bad.npz"):
        _choose(train_vocoder, hp, dirs, [])
    monkeypatch.setenv("TWV_VOCODER_CORPUS", "host")
    lines = []
    reader, route = _choose(train_vocoder, hp, dirs, lines)
    assert route == "host" and type(reader) is train_vocoder.DataFeederWavenet and not lines
    monkeypatch.setenv("TWV_VOCODER_CORPUS", "pinned")
    with pytest.raises(ValueError, match="TWV_VOCODER_CORPUS"):
        _choose(train_vocoder, hp, dirs, [])
