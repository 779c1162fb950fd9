"""What the WaveNet feed tests share (tests/test_wavenet_feed_cpu.py, tests/test_wavenet_feed_gpu.py): small corpora of npz examples
written with np.savez from a seeded generator, and the comparison of two feeders' batches bit for bit."""
import numpy as np

RECEPTIVE_FIELD = 10
REFILLS = 3


def feed_hp(hop_size=5, num_mels=4, frames=4, batch=3, extra=2):
    """default hparams at a small geometry; sample_size is `frames` frames' worth plus `extra` samples (floored away by the feeders)"""
    import twvk_amd
    hp = twvk_amd.default_hparams()
    hp.hop_size, hp.num_mels, hp.sample_size, hp.wavenet_batch_size = hop_size, num_mels, frames * hop_size + extra, batch
    return hp


def write_corpus(root, hp, frame_counts, seed=0):
    """one directory per entry of frame_counts, one npz per frame count in it (audio (frames * hop,), mel (frames, num_mels), and a
    'linear' array the feeders must never need): the directories' paths"""
    rng = np.random.RandomState(seed)
    dirs = []
    for spk, counts in enumerate(frame_counts):
        d = root / ("spk%d" % spk)
        d.mkdir(parents=True)
        dirs.append(str(d))
        for i, frames in enumerate(counts):
            np.savez(str(d / ("utt%02d.npz" % i)), audio=rng.uniform(-1, 1, frames * hp.hop_size).astype(np.float32),
                     mel=rng.uniform(-4, 4, (frames, hp.num_mels)).astype(np.float32), linear=rng.randn(frames, 3).astype(np.float32))
    return dirs


# two directories x 7 utterances of 5 .. 40 frames, one per directory too short for the filter: at hop 5 and 4 frames per crop the
# filter asks for MORE than 20 samples, so 4 frames fail it by the strict inequality alone and 5 frames pass with two possible starts
SCHEDULE_COUNTS = ((5, 40, 4, 17, 9, 23, 31), (12, 4, 6, 38, 5, 27, 20))


def batches_to_cross(batch, refills=REFILLS):
    """a refill serves 32 batches (two directories: int(batch * 32 // 2) * 2 examples cut into batches): enough calls to see `refills`
    refills and one batch more"""
    return 32 * refills + 1


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_same_batch(got, want, where):
    for name, g, w in zip(("audio", "local_condition", "gc_ids"), got, want):
        assert same_bits(g, w), "%s: %s differs" % (where, name)
