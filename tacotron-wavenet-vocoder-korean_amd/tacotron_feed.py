"""What feeds a Tacotron training step: the reference's data feeder (datasets/datafeeder_tacotron.py) as an iterator, and the
staging of its batches on the device.

    feeder = DataFeederTacotron(data_dirs, hp, batch_size=32, batches_per_group=32, data_type='train', random_seed=123)
    stager = BatchStager(model.device, hp.num_mels, hp.num_freq)
    for examples, batch in staged_batches(feeder, stager):         # lists of load_example dicts in the reference's order, and the padded
        # device tensors twv_tacotron_batch_stage built of them (batch k + 1 is loaded, packed, copied and staged while step k runs)
        trainer.step(batch["inputs"], batch["input_lengths"], batch["speaker_id"], batch["mel_targets"], batch["linear_targets"], batch["loss_coeff"])

`prepare_batch` is datafeeder_tacotron.py:269-309 on the host; `pack_batch` lays a batch's ragged arrays into one buffer with no padding
and `stage_numpy` restates in numpy what the staging kernel makes of that buffer (the two agree bit for bit, tests/test_tacotron_feed_*).

The feeder keeps the reference's rules: the path filter (min_iters, max_iters, min_tokens), the last n_test paths of a directory as the
test set, per-directory offsets that start at 2 and a reshuffle on wrap-around, batches_per_group batches' worth of examples per group,
the initial_phase_step rule with data_ratio / main_data_greedy_factor, sort by frame count -> cut into batches -> shuffle the batches ->
shuffle inside a batch, targets padded to _round_up(max + 1, r), and the test feeder's static batch.  What differs:
  * paths are sorted before the seeded shuffle (`glob` order depends on the file system);
  * there is no TensorFlow queue and no feeder thread of the reference's kind: the feeder is a synchronous iterator, with an optional
    thread that keeps ONE batch ahead and cannot change the order (one thread, one queue);
  * with world > 1 ranks each rank takes every world-th path of a directory and seeds random_seed + rank, as train_vocoder's
    DataFeederWavenet does (the reference has one process);
  * a file that cannot be read (OSError, a cut-off or broken archive) is skipped, not deleted (the reference calls remove_file, on any
    exception); any other error of an example is raised; a directory none of whose examples passes the
    filter raises instead of looping for ever;
  * get_path_dict's black list for the "son" / "yuinna" directories is not restated: `any(check not in path ...)` over three patterns
    is true of every path, so it removes nothing.
PyTorch is used for pinned and device memory, streams and events only."""
import ctypes as C
import os
import queue
import threading
import zipfile
from collections import defaultdict
from glob import glob

import numpy as np

from .eval_tacotron import _round_up, load_example

# twv_tacotron_feed_row (include/twv_amd.h): eight 32-bit words
ROW_DTYPE = np.dtype([("token_offset", "<i8"), ("frame_offset", "<i8"), ("n_tokens", "<i4"), ("n_frames", "<i4"), ("speaker_id", "<i4"),
                      ("loss_coeff", "<f4")])
assert ROW_DTYPE.itemsize == 32
ROW_WORDS = 8
BATCH_KEYS = ("inputs", "input_lengths", "loss_coeff", "mel_targets", "linear_targets", "speaker_id")


# ---------------------------------------------------------------- the padded batch on the host
def target_frames(examples, r):
    """_prepare_targets: the longest frame count + 1, rounded up to a multiple of r (there is always a padding frame)"""
    return _round_up(max(len(ex["linear"]) for ex in examples) + 1, r)


def prepare_batch(examples, r, rng=None):
    """datafeeder_tacotron.py:269-309 `_prepare_batch` of the training kind on a list of load_example dicts: with `rng` the list is
    shuffled in place first (data_type == 'train'), then inputs are padded with 0 to the longest and both targets with 0 to
    _round_up(max frames + 1, r).  Returns a dict of numpy arrays under BATCH_KEYS."""
    if rng is not None:
        rng.shuffle(examples)
    t_in, t_out = max(len(ex["tokens"]) for ex in examples), target_frames(examples, r)

    def pad_target(t):
        t = np.asarray(t, np.float32)
        return np.pad(t, [(0, t_out - t.shape[0]), (0, 0)], mode='constant', constant_values=0)
    return {"inputs": np.stack([np.pad(np.asarray(ex["tokens"], np.int32), (0, t_in - len(ex["tokens"])), mode='constant', constant_values=0)
                                for ex in examples]),
            "input_lengths": np.asarray([len(ex["tokens"]) for ex in examples], np.int32),
            "loss_coeff": np.asarray([ex.get("loss_coeff", 1.0) for ex in examples], np.float32),
            "mel_targets": np.stack([pad_target(ex["mel"]) for ex in examples]),
            "linear_targets": np.stack([pad_target(ex["linear"]) for ex in examples]),
            "speaker_id": np.asarray([ex.get("speaker_id", 0) for ex in examples], np.int32)}


# ---------------------------------------------------------------- the packed buffer
def packed_layout(total_tokens, total_frames, batch, num_mels, num_freq, mel_shift=0, linear_shift=0):
    """where the four sections of a packed buffer start, in 32-bit words: tokens at 0, the mel and linear rows each at the next multiple
    of four words (+ mel_shift / linear_shift: a test's way to an odd start), the table at the next even word.  dict with tokens_at,
    mel_at, linear_at, table_at, words (the buffer's size), total_tokens, total_frames, batch."""
    def up(x, m):
        return (x + m - 1) // m * m
    mel_at = up(total_tokens, 4) + mel_shift
    linear_at = up(mel_at + total_frames * num_mels, 4) + linear_shift
    table_at = up(linear_at + total_frames * num_freq, 2)
    return {"tokens_at": 0, "mel_at": mel_at, "linear_at": linear_at, "table_at": table_at, "words": table_at + ROW_WORDS * batch,
            "total_tokens": total_tokens, "total_frames": total_frames, "batch": batch}


def batch_layout(examples, num_mels, num_freq, mel_shift=0, linear_shift=0):
    return packed_layout(sum(len(ex["tokens"]) for ex in examples), sum(len(ex["linear"]) for ex in examples), len(examples), num_mels, num_freq,
                         mel_shift, linear_shift)


def pack_batch(examples, num_mels, num_freq, out=None, mel_shift=0, linear_shift=0):
    """the ragged arrays of `examples`, in order and with no padding, in one buffer of 32-bit words: (buffer, layout).  out: a uint32
    array of at least layout["words"] words to pack into (the stager's pinned memory); a new array when None.  Words between the
    sections are not written."""
    lay = batch_layout(examples, num_mels, num_freq, mel_shift, linear_shift)
    if out is None:
        out = np.zeros(lay["words"], np.uint32)
    if out.dtype != np.uint32 or out.ndim != 1 or out.size < lay["words"]:
        raise ValueError("out must be a flat uint32 array of at least %d words" % lay["words"])
    tokens = out[lay["tokens_at"]:lay["tokens_at"] + lay["total_tokens"]].view(np.int32)
    mel = out[lay["mel_at"]:lay["mel_at"] + lay["total_frames"] * num_mels].view(np.float32).reshape(lay["total_frames"], num_mels)
    lin = out[lay["linear_at"]:lay["linear_at"] + lay["total_frames"] * num_freq].view(np.float32).reshape(lay["total_frames"], num_freq)
    table = out[lay["table_at"]:lay["table_at"] + ROW_WORDS * len(examples)].view(ROW_DTYPE)
    tok_at = frame_at = 0
    for n, ex in enumerate(examples):
        nt, nf = len(ex["tokens"]), len(ex["linear"])
        if np.shape(ex["mel"]) != (nf, num_mels) or np.shape(ex["linear"]) != (nf, num_freq):
            raise ValueError("example %d: mel %s and linear %s must be (%d, %d) and (%d, %d)" % (n, np.shape(ex["mel"]), np.shape(ex["linear"]), nf, num_mels, nf, num_freq))
        tokens[tok_at:tok_at + nt] = ex["tokens"]
        mel[frame_at:frame_at + nf] = ex["mel"]
        lin[frame_at:frame_at + nf] = ex["linear"]
        table[n] = (tok_at, frame_at, nt, nf, ex.get("speaker_id", 0), ex.get("loss_coeff", 1.0))
        tok_at += nt
        frame_at += nf
    return out, lay


def stage_numpy(buf, lay, t_in, t_out, num_mels, num_freq):
    """what twv_tacotron_batch_stage writes for the packed buffer (buf, lay), in numpy: the dict of prepare_batch.  Every element is
    assigned: the outputs start full of a NaN / -1 pattern and the padding is stored."""
    buf = np.asarray(buf, np.uint32)
    table = buf[lay["table_at"]:lay["table_at"] + ROW_WORDS * lay["batch"]].view(ROW_DTYPE)
    N = lay["batch"]
    if int(table["n_tokens"].max()) > t_in or int(table["n_frames"].max()) > t_out:
        raise ValueError("t_in = %d / t_out = %d do not hold the longest utterance (%d tokens, %d frames)"
                         % (t_in, t_out, int(table["n_tokens"].max()), int(table["n_frames"].max())))
    out = {"inputs": np.full((N, t_in), -1, np.int32), "input_lengths": table["n_tokens"].astype(np.int32),
           "loss_coeff": table["loss_coeff"].astype(np.float32), "mel_targets": np.full((N, t_out, num_mels), np.nan, np.float32),
           "linear_targets": np.full((N, t_out, num_freq), np.nan, np.float32), "speaker_id": table["speaker_id"].astype(np.int32)}
    for n in range(N):
        to, fo, nt, nf = (int(table[k][n]) for k in ("token_offset", "frame_offset", "n_tokens", "n_frames"))
        out["inputs"][n, :nt] = buf[lay["tokens_at"] + to:lay["tokens_at"] + to + nt].view(np.int32)
        out["inputs"][n, nt:] = 0
        for key, at, C_ in (("mel_targets", lay["mel_at"], num_mels), ("linear_targets", lay["linear_at"], num_freq)):
            out[key][n, :nf] = buf[at + fo * C_:at + (fo + nf) * C_].view(np.float32).reshape(nf, C_)
            out[key][n, nf:] = 0.0
    return out


def stage_packed(packed_dev, table_host, lay, t_in, t_out, num_mels, num_freq, out=None, fill_nan=False):
    """twv_tacotron_batch_stage on the current stream: packed_dev (an int32 device tensor holding the packed buffer), table_host (the
    buffer's table in host memory, a ROW_DTYPE array) -> the dict of BATCH_KEYS as device tensors.  fill_nan: the outputs start as NaN /
    -1 (a test's proof that every element is written)."""
    import torch
    from . import _lib
    from .tacotron import _ptr, _stream
    dev, N = packed_dev.device, lay["batch"]
    table_host = np.ascontiguousarray(table_host)
    assert table_host.dtype == ROW_DTYPE and table_host.shape == (N,), (table_host.dtype, table_host.shape)
    with torch.cuda.device(dev):
        if out is None:
            def new(shape, dtype):
                if not fill_nan:
                    return torch.empty(shape, dtype=dtype, device=dev)
                return torch.full(shape, float("nan") if dtype == torch.float32 else -1, dtype=dtype, device=dev)
            out = {"inputs": new((N, t_in), torch.int32), "input_lengths": new((N,), torch.int32), "loss_coeff": new((N,), torch.float32),
                   "mel_targets": new((N, t_out, num_mels), torch.float32), "linear_targets": new((N, t_out, num_freq), torch.float32),
                   "speaker_id": new((N,), torch.int32)}
        _lib.check(_lib.lib().twv_tacotron_batch_stage(
            _ptr(packed_dev), table_host.ctypes.data_as(C.c_void_p), int(packed_dev.numel()), lay["tokens_at"], lay["mel_at"], lay["linear_at"],
            lay["table_at"], lay["total_tokens"], lay["total_frames"], N, int(t_in), int(t_out), int(num_mels), int(num_freq), _ptr(out["inputs"]),
            _ptr(out["input_lengths"]), _ptr(out["mel_targets"]), _ptr(out["linear_targets"]), _ptr(out["loss_coeff"]), _ptr(out["speaker_id"]),
            _stream()))
    return out


class BatchStager(object):
    """Batches onto the device through two packed buffers that alternate: a batch is packed into pinned memory, copied ONCE on the feed
    stream and staged there by twv_tacotron_batch_stage; the stream the caller computes on waits for the staging's event.  While the
    caller's step k runs, batch k + 1 can be packed, copied and staged (from a prefetch thread, or simply before the step is waited
    for): a pinned buffer is packed again only after its own copy has finished, a device buffer is overwritten only by the feed stream,
    after the staging that read it."""

    def __init__(self, device, num_mels, num_freq, words=0):
        import torch
        self.device, self.num_mels, self.num_freq = torch.device(device), int(num_mels), int(num_freq)
        with torch.cuda.device(self.device):
            self.stream = torch.cuda.Stream()
            self._copied = [torch.cuda.Event(), torch.cuda.Event()]
        self._pinned, self._dev, self._k = [None, None], [None, None], 0
        if words:
            self.reserve(words)

    def reserve(self, words):
        """both pairs of buffers at `words` 32-bit words at least (packed_layout(...)["words"] of the largest batch)"""
        import torch
        for s in range(2):
            if self._pinned[s] is None or self._pinned[s].numel() < words:
                self._copied[s].synchronize()
                with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
                    self._pinned[s] = torch.empty(int(words), dtype=torch.int32).pin_memory()
                    self._dev[s] = torch.empty(int(words), dtype=torch.int32, device=self.device)

    def stage(self, examples, r, t_in=None, t_out=None, wait=True):
        """examples (load_example dicts, in the batch's order) -> the padded batch as device tensors (BATCH_KEYS), plus "event".  t_in /
        t_out: the padded sizes, by default prepare_batch's.  wait: the current stream waits for the staging here; with wait=False the
        caller calls `ready(batch)` on the stream that will read it."""
        import torch
        lay = batch_layout(examples, self.num_mels, self.num_freq)
        self.reserve(lay["words"])
        s = self._k & 1
        self._k += 1
        self._copied[s].synchronize()                         # (the pinned buffer's last copy has left it)
        host = self._pinned[s].numpy().view(np.uint32)
        pack_batch(examples, self.num_mels, self.num_freq, out=host)
        t_in = max(len(ex["tokens"]) for ex in examples) if t_in is None else int(t_in)
        t_out = target_frames(examples, r) if t_out is None else int(t_out)
        table = host[lay["table_at"]:lay["table_at"] + ROW_WORDS * lay["batch"]].view(ROW_DTYPE)
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
            self._dev[s][:lay["words"]].copy_(self._pinned[s][:lay["words"]], non_blocking=True)
            self._copied[s].record(self.stream)
            out = stage_packed(self._dev[s], table, lay, t_in, t_out, self.num_mels, self.num_freq)
            out["event"] = torch.cuda.Event()
            out["event"].record(self.stream)
        if wait:
            self.ready(out)
        return out

    def ready(self, batch):
        """the current stream waits for the batch's staging; its tensors, allocated on the feed stream, are made known to this one"""
        import torch
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(batch["event"])
        for k in BATCH_KEYS:
            batch[k].record_stream(cur)
        return batch


# ---------------------------------------------------------------- the feeder
def get_path_dict(data_dirs, hp, data_type, n_test, rng, skip_path_filter=False, rank=0, world=1, log=None):
    """datafeeder_tacotron.py:28-71: {directory: its example paths}.  Sorted, (rank's share,) shuffled with `rng` for 'train', filtered by
    frame and token counts unless skip_path_filter, then all but the last n_test ('train') or the last n_test ('test')."""
    if data_type not in ("train", "test"):
        raise ValueError(" [!] Unkown data_type: {}".format(data_type))
    r = hp.reduction_factor
    min_n_frame, max_n_frame = r * hp.min_iters, r * hp.max_iters - r
    path_dict = {}
    for d in data_dirs:
        paths = sorted(glob("{}/*.npz".format(d)))
        if not paths:
            raise ValueError("no .npz examples in %s" % d)
        if world > 1 and len(paths) >= world:               # data-parallel ranks read disjoint examples
            paths = paths[rank::world]
        if data_type == "train":
            rng.shuffle(paths)
        if not skip_path_filter:
            kept = []
            for p in paths:
                data = np.load(p)
                n_frame, n_token = data["linear"].shape[0], len(data["tokens"])
                if min_n_frame <= n_frame <= max_n_frame and n_token >= hp.min_tokens:
                    kept.append(p)
            if log is not None:
                log(" [%s] Loaded metadata for %d examples (%d before the filter)" % (d, len(kept), len(paths)))
            paths = kept
        path_dict[d] = paths[:-n_test] if data_type == "train" else paths[-n_test:]
    return path_dict


class DataFeederTacotron(object):
    """datafeeder_tacotron.py:75-266 as a synchronous iterator (see the module docstring for what is kept and what differs).
    next_examples() gives the next batch as a list of load_example dicts in feed order -- shuffled inside the batch for 'train' -- and
    next_batch() that batch padded by prepare_batch.  A 'test' feeder gives its static batch every time."""

    def __init__(self, data_dirs, hp, batch_size, batches_per_group, data_type="train", random_seed=123, skip_path_filter=False, rank=0,
                 world=1, start_step=0, path_dict=None, log=None):
        self._hp = hp
        self._step = int(start_step)
        self._offset = defaultdict(lambda: 2)
        self._batches_per_group = int(batches_per_group)
        self.rng = np.random.RandomState(random_seed + rank)
        self.data_type, self.batch_size = data_type, int(batch_size)
        self.min_tokens = hp.min_tokens
        self.min_n_frame = hp.reduction_factor * hp.min_iters
        self.max_n_frame = hp.reduction_factor * hp.max_iters - hp.reduction_factor
        self.skip_path_filter = bool(skip_path_filter)
        # (path_dict given: a test's stand-in for the directory scan, used as it is)
        self.path_dict = path_dict if path_dict is not None else get_path_dict(data_dirs, hp, data_type, self.batch_size, self.rng,
                                                                               self.skip_path_filter, rank, world, log)
        self.data_dirs = list(self.path_dict.keys())
        self.data_dir_to_id = {d: i for i, d in enumerate(self.data_dirs)}
        weight = {d: 1. for d in self.data_dirs}
        if hp.main_data_greedy_factor > 0 and any(main in d for d in self.data_dirs for main in hp.main_data):
            for main in hp.main_data:
                for d in self.data_dirs:
                    if main in d:
                        weight[d] += hp.main_data_greedy_factor
        z = sum(weight.values())
        self.data_ratio = {d: w / z for d, w in weight.items()}
        self.is_multi_speaker = len(self.data_dirs) > 1
        self._batches = []
        self.static_batch = None
        if data_type == "test":
            examples = []
            while len(examples) < self.batch_size:
                for d in self.data_dirs:
                    examples.append(self._get_next_example(d))
                    if len(examples) >= self.batch_size:
                        break
            self.static_batch = examples

    def _get_next_example(self, data_dir):
        """datafeeder_tacotron.py:228-266: the directory's next readable example (with skip_path_filter, the next that passes the filter
        here)"""
        data_paths, skipped = self.path_dict[data_dir], None
        for _ in range(4 * len(data_paths) + 8):
            if self._offset[data_dir] >= len(data_paths):
                self._offset[data_dir] = 0
                if self.data_type == "train":
                    self.rng.shuffle(data_paths)
            if not data_paths:
                break
            data_path = data_paths[self._offset[data_dir]]
            self._offset[data_dir] += 1
            if not os.path.exists(data_path):
                continue
            try:
                ex = load_example(data_path, self.data_dir_to_id[data_dir])
            except (OSError, EOFError, zipfile.BadZipFile) as e:    # an unreadable or cut-off file is skipped (the reference removes it);
                skipped = skipped or "%s: %r" % (data_path, e)      # anything else -- a missing key, a wrong shape -- is raised
                continue
            if not self.skip_path_filter:
                return ex
            if self.min_n_frame <= ex["linear"].shape[0] <= self.max_n_frame and len(ex["tokens"]) > self.min_tokens:
                return ex
        raise ValueError("no usable example in %s%s" % (data_dir, "" if skipped is None else " (first unreadable file: %s)" % skipped))

    def _next_group(self):
        """datafeeder_tacotron.py:194-217: a group's batches, each a list of examples"""
        if self.static_batch is not None:
            return [list(self.static_batch) for _ in range(self._batches_per_group)]
        hp, n = self._hp, self.batch_size
        examples = []
        for data_dir in self.data_dirs:
            if hp.initial_data_greedy:
                if self._step < hp.initial_phase_step and any("krbook" in d for d in self.data_dirs):
                    data_dir = [d for d in self.data_dirs if "krbook" in d][0]
            if self._step < hp.initial_phase_step:
                count = int(n * self._batches_per_group // len(self.data_dirs))
            else:
                count = int(n * self._batches_per_group * self.data_ratio[data_dir])
            examples.extend(self._get_next_example(data_dir) for _ in range(count))
        examples.sort(key=lambda ex: len(ex["linear"]))
        batches = [examples[i:i + n] for i in range(0, len(examples), n)]
        self.rng.shuffle(batches)
        return batches

    def next_examples(self):
        if not self._batches:
            self._batches = self._next_group()
        batch = self._batches.pop(0)
        if self.data_type == "train":
            self.rng.shuffle(batch)                        # (_prepare_batch's shuffle, made here so that the order is the batch's)
        self._step += 1
        return batch

    def next_batch(self):
        return prepare_batch(self.next_examples(), self._hp.reduction_factor)

    def example_batches(self, count=None, prefetch=False):
        """iterates over next_examples(): `count` batches, or for ever.  prefetch: a thread loads one batch ahead; the batches and their
        order are the same (one producer, one queue), and the feeder must not be used otherwise while the iteration lasts."""
        return _iterate(self.next_examples, count, prefetch)


def _iterate(next_item, count=None, prefetch=False):
    """next_item() `count` times (or for ever), in order; prefetch: from ONE thread that stays one item ahead of the consumer.  What the
    producer raises is raised where the consumer asks for that item."""
    if not prefetch:
        k = 0
        while count is None or k < count:
            yield next_item()
            k += 1
        return
    q, stop = queue.Queue(maxsize=1), threading.Event()

    def put(item):
        while not stop.is_set():
            try:
                q.put(item, timeout=0.05)
                return
            except queue.Full:
                pass

    def produce():
        k = 0
        try:
            while not stop.is_set() and (count is None or k < count):
                put((next_item(), None))
                k += 1
        except BaseException as e:                  # noqa: BLE001 -- handed to the consumer
            put((None, e))
    t = threading.Thread(target=produce, daemon=True)
    t.start()
    try:
        k = 0
        while count is None or k < count:
            item, err = q.get()
            if err is not None:
                raise err
            yield item
            k += 1
    finally:
        stop.set()
        t.join()


def staged_batches(feeder, stager, count=None, prefetch=True):
    """the feeder's batches on the device, in the feeder's order: (examples, batch) with batch = stager.stage(examples, r) made ready for
    the current stream.  prefetch: one thread loads, packs, copies and stages batch k + 1 (on the stager's stream) while the caller's
    step k runs."""
    r = feeder._hp.reduction_factor

    def next_item():
        import torch
        examples = feeder.next_examples()
        with torch.cuda.device(stager.device):
            return examples, stager.stage(examples, r, wait=False)
    for examples, batch in _iterate(next_item, count, prefetch):
        yield examples, stager.ready(batch)
