"""What feeds a WaveNet training step when the corpus lives on the device.

    index = CorpusIndex(data_dirs, batch_size, receptive_field, gc_enable, hp, rank, world)     # reads every npz ONCE, host only
    feeder = DeviceFeederWavenet(index, device)                                                  # uploads the two pools once
    audio, lc, gc = feeder.next_batch()                         # device tensors, the bits of DataFeederWavenet.next_batch()
    feeder = PrefetchFeeder(DataFeederWavenet(...))             # the host feeder one batch ahead, for corpora that do not fit

train_vocoder.DataFeederWavenet reads 32 batches' worth of whole npz files in one burst, on the host, to keep one `sample_size` crop of
each.  Here every example's audio and mel rows are packed once into two float32 pools; the schedule -- which example, which start frame,
in which batch -- is drawn on the host with the host feeder's own generators, and ONE kernel (twv_wavenet_crop_stage) cuts a batch's
crops out of the pools.  The host's share of a step is the drawing of B integers and a copy of 8 B bytes.

The pools: every example's audio starts at a multiple of four floats of the audio pool (the words between two examples are zero and never
read), the mel rows are packed densely in the mel pool.  The table has one twv_wavenet_feed_row per example (include/twv_amd.h).

The schedule is DataFeederWavenet's, draw for draw: CorpusIndex keeps, per directory, the list of its examples in the order of the
sorted basenames (a rank's share: every world-th), an offset that starts at 2, `rng.shuffle` of that list on wrap-around,
int(n * 32 // len(data_dirs)) examples per directory per refill with the `time_steps > max(sample_size, receptive_field)` filter
consuming an offset when it skips, np.random.randint(0, frames - max_frames + 1) from the GLOBAL generator per kept example, in the order
the host feeder calls it, `rng.shuffle` of the refill's examples, and the cut into batches.  Both shuffles permute Python lists of the
same lengths as the host feeder's, so they consume the same draws and give the same permutations.

What differs from the host feeder, on purpose: the corpus is a SNAPSHOT.  A file deleted during the run is still served (the host
feeder's os.path.exists would skip it), and a file that breaks crop_example's assertion (len(audio) = hop_size * len(mel)) fails the
pack at once, with its name, also when it is too short to be cropped ever.
PyTorch is used for pinned and device memory, streams and events only."""
import ctypes as C
import os
import queue
import threading
from glob import glob

import numpy as np

from .train_vocoder import ensure_divisible

# twv_wavenet_feed_row (include/twv_amd.h): six 32-bit words
ROW_DTYPE = np.dtype([("audio_offset", "<i8"), ("mel_offset", "<i8"), ("n_frames", "<i4"), ("speaker_id", "<i4")])
assert ROW_DTYPE.itemsize == 24
AUDIO_ALIGN = 4                  # floats: every example's audio starts on a 16-byte boundary of the pool
UPLOAD_CHUNK = 16 << 20          # floats per piece of the pools' upload (64 MiB of pinned memory)


class CorpusTooLarge(ValueError):
    """the pack was given a byte limit and passed it"""


class _Pool(object):
    """a float32 array that grows by doubling"""

    def __init__(self):
        self.buf, self.n = np.zeros(1 << 16, np.float32), 0

    def append(self, a, align=1):
        at = -(-self.n // align) * align
        if at + a.size > self.buf.size:
            grown = np.zeros(max(2 * self.buf.size, at + a.size), np.float32)
            grown[:self.n] = self.buf[:self.n]
            self.buf = grown
        self.buf[at:at + a.size] = a
        self.n = at + a.size
        return at

    def array(self):
        return self.buf[:self.n]


class CorpusIndex(object):
    """The corpus packed on the host and DataFeederWavenet's schedule over it (host only; see the module docstring).

    audio_pool, mel_pool: the two float32 pools; table: a ROW_DTYPE array, one row per example; names[i]: example i's path.
    next_picks() -> (example, start_frame, speaker): three int32 arrays of length batch_size, the next batch of the host feeder.
    max_bytes: CorpusTooLarge is raised as soon as the two pools hold more."""

    def __init__(self, data_dirs, batch_size, receptive_field, gc_enable=False, hp=None, rank=0, world=1, max_bytes=None):
        if hp is None:
            from .hparams import hparams as hp
        self.data_dirs = list(data_dirs)
        self.batch_size = int(batch_size)
        self.receptive_field = receptive_field
        self.hop_size, self.num_mels = int(hp.hop_size), int(hp.num_mels)
        self.sample_size = ensure_divisible(hp.sample_size, self.hop_size, True)
        self.max_frames = self.sample_size // self.hop_size
        self.gc_enable = gc_enable
        self.rng = np.random.RandomState(123 + rank)
        self._offset = {}
        self.data_dir_to_id = {d: i for i, d in enumerate(self.data_dirs)}
        path_dict = {d: sorted(os.path.basename(p) for p in glob("{}/*.npz".format(d))) for d in self.data_dirs}
        for d, paths in path_dict.items():
            if not paths:
                raise ValueError("no .npz examples in %s" % d)
            if world > 1 and len(paths) >= world:                       # a directory with fewer files than ranks is shared whole
                path_dict[d] = paths[rank::world]
        audio, mel, rows, self.names, self.path_dict = _Pool(), _Pool(), [], [], {}
        for d, paths in path_dict.items():
            self.path_dict[d] = []                                      # the directory's example numbers, in the feeder's order
            self._offset[d] = 2
            for name in paths:
                path = os.path.join(d, name)
                a, m = self._load(path)
                rows.append((audio.append(a, AUDIO_ALIGN), mel.append(m.reshape(-1)), m.shape[0], self.data_dir_to_id[d]))
                self.path_dict[d].append(len(self.names))
                self.names.append(path)
                if max_bytes is not None and 4 * (audio.n + mel.n) > max_bytes:
                    raise CorpusTooLarge("the corpus does not fit: %d bytes packed after %d of %d examples, the limit is %d"
                                         % (4 * (audio.n + mel.n), len(self.names), sum(len(p) for p in path_dict.values()), max_bytes))
        self.audio_pool, self.mel_pool = audio.array(), mel.array()
        self.table = np.array(rows, ROW_DTYPE)
        self._rank, self._first_order = rank, {d: list(p) for d, p in self.path_dict.items()}
        self._batches = []

    def rewind(self):
        """the schedule of a newly made index again (generator, offsets, orders), without another pack"""
        self.rng = np.random.RandomState(123 + self._rank)
        for d, order in self._first_order.items():
            self.path_dict[d][:] = order
            self._offset[d] = 2
        self._batches = []

    def _load(self, path):
        """one npz, read once, the keys 'audio' and 'mel' only -> (audio (T,), mel (frames, num_mels)) as float32"""
        with np.load(path) as data:
            a, m = np.asarray(data['audio']).reshape(-1), np.asarray(data['mel'])
        if m.ndim != 2 or m.shape[1] != self.num_mels:
            raise ValueError("%s: mel must be (frames, %d), got %s" % (path, self.num_mels, m.shape))
        if len(m) == 0 or len(a) % len(m) != 0 or len(a) // len(m) != self.hop_size:         # crop_example's assertion
            raise ValueError("%s: %d audio samples and %d mel frames are not hop_size = %d samples per frame" % (path, len(a), len(m), self.hop_size))
        return a.astype(np.float32), m.astype(np.float32)

    @property
    def n_examples(self):
        return len(self.names)

    @property
    def packed_bytes(self):
        return 4 * (self.audio_pool.size + self.mel_pool.size)

    def _next_pick(self, data_dir):
        """DataFeederWavenet._get_next_example without the files: (example, start frame, speaker)"""
        examples = self.path_dict[data_dir]
        min_len = max(self.sample_size, self.receptive_field)
        for _ in range(4 * len(examples) + 8):
            if self._offset[data_dir] >= len(examples):
                self._offset[data_dir] = 0
                self.rng.shuffle(examples)
            ex = examples[self._offset[data_dir]]
            self._offset[data_dir] += 1
            frames = int(self.table["n_frames"][ex])
            if frames * self.hop_size > min_len:
                return ex, np.random.randint(0, frames - self.max_frames + 1), self.data_dir_to_id[data_dir]
        raise ValueError("no example in %s is longer than %d samples" % (data_dir, min_len))

    def next_picks(self):
        if not self._batches:
            n = self.batch_size
            picks = []
            for d in self.data_dirs:
                picks.extend(self._next_pick(d) for _ in range(int(n * 32 // len(self.data_dirs))))
            self.rng.shuffle(picks)
            self._batches = [picks[i:i + n] for i in range(0, len(picks) - n + 1, n)]
        batch = np.asarray(self._batches.pop(0), np.int32).reshape(-1, 3)
        return batch[:, 0].copy(), batch[:, 1].copy(), batch[:, 2].copy()


def crop_stage(audio_pool, mel_pool, table_host, table_dev, picks_host, picks_dev, frames, hop_size, num_mels, out=None):
    """twv_wavenet_crop_stage on the current stream.  audio_pool / mel_pool: float32 device tensors; table_host: a ROW_DTYPE array,
    table_dev: the same bytes on the device; picks_host (B, 2) int32 array, picks_dev: the same on the device.  out: (audio (B, frames *
    hop_size), local_condition (B, frames, num_mels), gc_ids (B)) to write into; new tensors when None.  Returns the three tensors."""
    import torch
    from . import _lib
    from .wavenet import _ptr, _stream
    dev = audio_pool.device
    table_host, picks_host = np.ascontiguousarray(table_host), np.ascontiguousarray(picks_host)
    assert table_host.dtype == ROW_DTYPE and table_host.ndim == 1, (table_host.dtype, table_host.shape)
    assert picks_host.dtype == np.int32 and picks_host.ndim == 2 and picks_host.shape[1] == 2, (picks_host.dtype, picks_host.shape)
    B = picks_host.shape[0]
    assert table_dev.numel() * table_dev.element_size() == table_host.nbytes and picks_dev.numel() * picks_dev.element_size() == picks_host.nbytes
    with torch.cuda.device(dev):
        if out is None:
            out = (torch.empty((B, frames * hop_size), dtype=torch.float32, device=dev), torch.empty((B, frames, num_mels), dtype=torch.float32, device=dev),
                   torch.empty((B,), dtype=torch.int32, device=dev))
        audio, lc, gc = out
        _lib.check(_lib.lib().twv_wavenet_crop_stage(
            _ptr(audio_pool), int(audio_pool.numel()), _ptr(mel_pool), int(mel_pool.numel()), table_host.ctypes.data_as(C.c_void_p), _ptr(table_dev),
            int(table_host.shape[0]), picks_host.ctypes.data_as(C.c_void_p), _ptr(picks_dev), B, int(frames), int(hop_size), int(num_mels),
            _ptr(audio), _ptr(lc), _ptr(gc), _stream()))
    return audio, lc, gc


class DeviceFeederWavenet(object):
    """DataFeederWavenet's batches cut on the device from the resident corpus of `index` (a CorpusIndex): next_batch() -> (audio (B,
    sample_size), local_condition (B, frames, num_mels) float32, speaker ids (B) int32) as DEVICE tensors on the current stream, bit for
    bit what the host feeder returns for the same directories, seeds, rank and world.  The two pools are uploaded once, through one
    pinned buffer in pieces; the table is kept on both sides; a batch costs one copy of its (B, 2) picks and one kernel launch."""

    def __init__(self, index, device):
        import torch
        self.index, self.device = index, torch.device(device)
        self.table = np.ascontiguousarray(index.table)
        with torch.cuda.device(self.device):
            self.audio_pool, self.mel_pool = self._upload(index.audio_pool), self._upload(index.mel_pool)
            self.table_dev = torch.from_numpy(self.table.view(np.int32).copy()).to(self.device)
            # the picks go up through two pinned slots that alternate: a slot is written again only after its own copy has left it
            self._pinned = [torch.empty((index.batch_size, 2), dtype=torch.int32).pin_memory() for _ in range(2)]
            self._copied = [torch.cuda.Event(), torch.cuda.Event()]
        self._k = 0

    def _upload(self, pool):
        import torch
        dev = torch.empty(max(int(pool.size), 1), dtype=torch.float32, device=self.device)
        if pool.size:
            pinned = torch.empty(min(int(pool.size), UPLOAD_CHUNK), dtype=torch.float32).pin_memory()
            host = pinned.numpy()
            for at in range(0, pool.size, UPLOAD_CHUNK):
                n = min(UPLOAD_CHUNK, pool.size - at)
                host[:n] = pool[at:at + n]
                dev[at:at + n].copy_(pinned[:n], non_blocking=True)
                torch.cuda.current_stream(self.device).synchronize()    # (the one pinned buffer is filled again next)
        return dev

    def stage(self, example, start_frame):
        """the crops of the given picks as device tensors (audio, local_condition, gc_ids)"""
        import torch
        ix = self.index
        s = self._k & 1
        self._k += 1
        self._copied[s].synchronize()
        picks = self._pinned[s].numpy()
        picks[:, 0], picks[:, 1] = example, start_frame
        with torch.cuda.device(self.device):
            picks_dev = self._pinned[s].to(self.device, non_blocking=True)
            self._copied[s].record()
            return crop_stage(self.audio_pool, self.mel_pool, self.table, self.table_dev, picks, picks_dev, ix.max_frames, ix.hop_size, ix.num_mels)

    def next_batch(self):
        example, start_frame, _ = self.index.next_picks()
        return self.stage(example, start_frame)


class PrefetchFeeder(object):
    """Any feeder behind ONE thread that stays one batch ahead: next_batch() returns the wrapped feeder's batches in its order (one
    producer, one queue).  Every draw of the feeder's generators -- the global np.random among them -- is made in that thread: seed
    before the first next_batch() (the thread starts there) and draw nothing from np.random elsewhere while the feeder is in use.  What
    the wrapped feeder raises at batch k is raised by the k-th next_batch(), and by every later one."""

    def __init__(self, feeder):
        self.feeder = feeder
        self._q, self._stop, self._thread, self._error = queue.Queue(maxsize=1), threading.Event(), None, None

    def _put(self, item):
        while not self._stop.is_set():
            try:
                self._q.put(item, timeout=0.05)
                return
            except queue.Full:
                pass

    def _produce(self):
        try:
            while not self._stop.is_set():
                self._put((self.feeder.next_batch(), None))
        except BaseException as e:                  # noqa: BLE001 -- handed to the consumer
            self._put((None, e))

    def next_batch(self):
        if self._error is not None:
            raise self._error
        if self._thread is None:
            self._thread = threading.Thread(target=self._produce, daemon=True)
            self._thread.start()
        batch, err = self._q.get()
        if err is not None:
            self._error = err
            raise err
        return batch

    def close(self):
        """stops the thread (a batch it had ready is dropped)"""
        self._stop.set()
        if self._thread is not None:
            self._thread.join()
            self._thread = None
        if self._error is None:
            self._error = RuntimeError("the feeder is closed")

    def __del__(self):
        try:
            self._stop.set()
        except Exception:
            pass
