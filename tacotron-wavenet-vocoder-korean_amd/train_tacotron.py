"""train_tacotron.py of the reference (train_tacotron.py:110-302) on the MI355X path: preprocess -> TRAIN -> eval_tacotron -> synthesizer.

    python -m twvk_amd.train_tacotron --data_paths D1,D2 [--log_dir logdir-tacotron] [--load_path DIR | --initialize_path DIR]
        [--batch_size 32] [--num_test_per_speaker 2] [--random_seed 123] [--summary_interval N] [--test_interval N]
        [--checkpoint_interval N] [--skip_path_filter false]  [--num_steps N] [--training true]

The flags are the reference's (train_tacotron.py:256-280); --slack_url and --git are accepted and ignored.  Extensions, as train_vocoder
has them: --num_steps (the reference runs until it is stopped), --training false (the evaluation-graph step: frozen batch norm, no
dropout) and main(argv, hp=None, log=print) for tests.  Launched with several ranks (RANK / WORLD_SIZE / LOCAL_RANK, one process per
GPU) the step is data-parallel (TacotronTrainer.step): rank 0 decides the directories, writes checkpoints, summaries and
test outputs; every rank reads its own share of the examples.

The loop is the reference's `train()`: the directories and params.json of prepare_dirs (utils/__init__.py:39-60); --load_path resumes
from the directory's latest checkpoint, --initialize_path restores another run's and resets the step to 0, both at once is an error;
one TacotronTrainer.step per iteration on the next batch of DataFeederTacotron (32 batches a group), staged on the device one batch
ahead (tacotron_feed.staged_batches); the log line with the step, sec/step, loss_without_coeff and their 100-step averages; 'Loss
Exploded' above 100 or at NaN; a checkpoint every --checkpoint_interval steps through TacotronTrainer.save (every one is kept, as
Saver(max_to_keep=None); Synthesizer.load reads them); at --summary_interval one JSON line to <model_dir>/stats.jsonl with the train and
test losses, their gap (test - train) and the learning rate; at --test_interval the train batch's first example (teacher-forced, in
inference mode) and the test feeder's static batch (forward_targets(teacher_forced=False) + add_loss, the reference's test_model) are
written as <train|test>-step-NNNNNNNNN-audioNNN.wav (Griffin-Lim on the linear output, audio.inv_linear_spectrogram + save_wav) and
-alignNNN.npy (T_in, decoder steps).

Out of scope:
  * alignment plots and the recovered text in them: the package has no text front end and no plotting; the alignment is saved as .npy;
  * TensorBoard event files: the summaries are the lines of stats.jsonl;
  * max_gradient_norm, the largest per-variable gradient norm of the reference's summary;
  * the copy of hparams.py into the model directory (params.json holds the values)."""
import argparse
import json
import math
import os
import time

import numpy as np

from .synthesizer import get_time, str2bool

BATCHES_PER_GROUP, TEST_BATCHES_PER_GROUP = 32, 8          # train_tacotron.py:136-137


def get_arguments(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument('--log_dir', default='logdir-tacotron')
    parser.add_argument('--data_paths', default='./data/moon,./data/son')
    parser.add_argument('--load_path', default=None)
    parser.add_argument('--initialize_path', default=None)
    parser.add_argument('--batch_size', type=int, default=32)
    parser.add_argument('--num_test_per_speaker', type=int, default=2)
    parser.add_argument('--random_seed', type=int, default=123)
    parser.add_argument('--summary_interval', type=int, default=100000)
    parser.add_argument('--test_interval', type=int, default=500)
    parser.add_argument('--checkpoint_interval', type=int, default=2000)
    parser.add_argument('--skip_path_filter', type=str2bool, default=False, help='Use only for debugging')
    parser.add_argument('--slack_url', help='accepted and ignored')
    parser.add_argument('--git', action='store_true', help='accepted and ignored')
    parser.add_argument('--num_steps', type=int, default=None, help='stop after this global step (extension; default: run until stopped)')
    parser.add_argument('--training', type=str2bool, default=True, help="false: the evaluation-graph step (extension)")
    config = parser.parse_args(argv)
    config.data_paths = config.data_paths.split(",")
    if config.load_path is not None and config.initialize_path is not None:
        raise ValueError(" [!] Only one of load_path and initialize_path should be set")
    return config


def prepare_dirs(config, hp, now=get_time):
    """utils/__init__.py:39-60: --load_path is the model directory and its params.json overrides the hyper-parameters; otherwise
    <log_dir>/<dataset names joined by +>_<time> is made and the hyper-parameters (with num_speakers) are written there.  Returns the
    model directory; called ONCE per run (the name carries the time)."""
    from .hparams import load_hparams, save_hparams
    datasets = [os.path.basename(p) for p in config.data_paths]
    if config.load_path:
        model_dir = config.load_path
        load_hparams(hp, model_dir)
    else:
        model_dir = os.path.join(config.log_dir, "{}_{}".format("+".join(datasets), now()))
        os.makedirs(model_dir, exist_ok=True)
        hp.num_speakers = len(datasets)
        save_hparams(model_dir, hp)
    return model_dir


def start_state(config, trainer, model_dir, log=print):
    """train_tacotron.py:177-197: where the run starts -- the step it resumes at (--load_path), 0 with another run's weights
    (--initialize_path), or 0 with the initial values the trainer already holds"""
    if config.load_path:
        step = trainer.restore(model_dir, verify=True)
        log('Resuming from checkpoint: %s at step %d' % (model_dir, step))
    elif config.initialize_path:
        trainer.restore(config.initialize_path, verify=True)
        trainer.global_step = 0
        log('Initialized from checkpoint: %s' % config.initialize_path)
        log(' [*] Global step is reset to {}'.format(trainer.global_step))
    else:
        log('Starting new training run')
    return trainer.global_step


class ValueWindow(object):
    """utils/__init__.py ValueWindow: the average of the last `size` values"""

    def __init__(self, size=100):
        self._size, self._values = size, []

    def append(self, x):
        self._values = self._values[-(self._size - 1):] + [x]

    @property
    def average(self):
        return sum(self._values) / max(1, len(self._values))


def _test_losses(model, batch):
    model.forward_targets(batch["inputs"], batch["input_lengths"], batch["speaker_id"], batch["mel_targets"], teacher_forced=False)
    return model.add_loss(batch["linear_targets"], batch["loss_coeff"])


def _save_outputs(model, hp, model_dir, prefix, step, linear, alignments):
    """save_and_plot (train_tacotron.py:84-107) without the plot: one wav and one alignment array per utterance"""
    from . import audio
    for idx in range(int(linear.shape[0])):
        base = os.path.join(model_dir, '{}-step-{:09d}'.format(prefix, step))
        wav = audio.inv_linear_spectrogram(linear[idx], hp, seed=0, device=model.device)
        audio.save_wav(wav[0], '{}-audio{:03d}.wav'.format(base, idx), hp.sample_rate)
        np.save('{}-align{:03d}.npy'.format(base, idx), alignments[idx].cpu().numpy())


def main(argv=None, hp=None, log=print):
    import torch
    from .hparams import hparams as default_hp, load_hparams
    from .tacotron import Tacotron
    from .tacotron_feed import BatchStager, DataFeederTacotron, prepare_batch, staged_batches
    from .tacotron_train import TacotronTrainer
    hp = default_hp if hp is None else hp
    config = get_arguments(argv)
    rank = int(os.environ.get("RANK", "0")); world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    dist = None
    if world > 1:                                                   # one process per GPU; gradients meet in TacotronTrainer.step
        import torch.distributed as dist
        torch.cuda.set_device(local_rank)
        if not dist.is_initialized():
            dist.init_process_group("nccl", device_id=torch.device("cuda:%d" % local_rank))
    # rank 0 decides the model directory (its name carries the time) and writes params.json; the others take its answer
    model_dir, setup_error = None, None
    if rank == 0:
        try:
            model_dir = prepare_dirs(config, hp)
        except Exception as e:                                      # the other ranks are waiting in the broadcast
            setup_error = e
    if dist is not None:
        box = [model_dir]
        dist.broadcast_object_list(box, src=0)                      # None = rank 0 could not set the run up: every rank leaves
        model_dir = box[0]
        if model_dir is not None and rank != 0:
            load_hparams(hp, model_dir)
    if setup_error is not None:
        raise setup_error
    if model_dir is None:
        return None
    data_dirs = config.data_paths
    num_speakers = len(data_dirs)
    hp.num_speakers = num_speakers
    num_test = config.num_test_per_speaker * num_speakers
    if num_speakers > 1 and hp.model_type not in ["deepvoice", "simple"]:
        raise ValueError("[!] Unkown model_type for multi-speaker: {}".format(hp.model_type))
    log(' [*] Checkpoint path: %s' % os.path.join(model_dir, 'model.ckpt'))
    log(' [*] Loading training data from: %s' % data_dirs)
    device = "cuda:%d" % local_rank
    model = Tacotron(hp, num_speakers, device=device)
    trainer = TacotronTrainer(model, randomly_initialized=config.initialize_path is None, training=config.training, seed=config.random_seed,
                              attention_gradients="any")          # whatever hparams.attention_type the model was built with
    trainer.init_weights(config.random_seed)                        # tf.global_variables_initializer (identical on every rank)
    start_step = start_state(config, trainer, model_dir, log)
    train_feeder = DataFeederTacotron(data_dirs, hp, config.batch_size, BATCHES_PER_GROUP, "train", config.random_seed, config.skip_path_filter,
                                      rank, world, start_step, log=log if rank == 0 else None)
    test_feeder = DataFeederTacotron(data_dirs, hp, num_test, TEST_BATCHES_PER_GROUP, "test", config.random_seed, config.skip_path_filter,
                                     start_step=start_step)
    r = hp.reduction_factor
    test_batch = prepare_batch(test_feeder.next_examples(), r)
    stager = BatchStager(device, hp.num_mels, hp.num_freq)
    time_window, loss_window = ValueWindow(100), ValueWindow(100)
    step, loss, losses = start_step, float("nan"), []
    batches = staged_batches(train_feeder, stager, prefetch=True)
    try:
        while config.num_steps is None or step < config.num_steps:
            start_time = time.time()
            failure = batch = None
            try:
                _, batch = next(batches)
            except Exception as e:                                  # noqa: BLE001 -- a rank that cannot feed must not leave the others in the all-reduce
                failure = e
            if failure is not None:
                trainer.step(None, None, None, None, None, failed=True)
                raise failure
            out = trainer.step(batch["inputs"], batch["input_lengths"], batch["speaker_id"], batch["mel_targets"], batch["linear_targets"],
                               batch["loss_coeff"])
            if dist is not None and trainer.peer_failure():
                raise RuntimeError("another rank failed at step %d" % (trainer.global_step + 1))
            step, loss = trainer.global_step, out["loss_without_coeff"]
            losses.append(loss)
            time_window.append(time.time() - start_time)
            loss_window.append(loss)
            log('Step %-7d [%.03f sec/step, loss=%.05f, avg_loss=%.05f]' % (step, time_window.average, loss, loss_window.average))
            if loss > 100 or math.isnan(loss):
                log('Loss exploded to %.05f at step %d!' % (loss, step))
                if dist is not None:                                # the loss is this rank's batch's: the peers are on their way into the next
                    trainer.step(None, None, None, None, None, failed=True)     # all-reduce and must find this rank there, flagged
                raise Exception('Loss Exploded')
            if rank != 0:
                continue
            if step % config.summary_interval == 0:
                log('Writing summary at step: %d' % step)
                test = _test_losses(model, test_batch)
                line = {"step": step, "learning_rate": trainer.last_learning_rate, "train": out, "test": test,
                        "gap_test-train": {k: test[k] - out[k] for k in ("mel_loss", "linear_loss", "loss_without_coeff")}}
                with open(os.path.join(model_dir, "stats.jsonl"), "a") as f:
                    f.write(json.dumps(line, sort_keys=True) + "\n")
            if step % config.checkpoint_interval == 0:
                log('Saving checkpoint to: %s-%d' % (os.path.join(model_dir, 'model.ckpt'), step))
                trainer.save(model_dir, step, max_to_keep=0)
            if step % config.test_interval == 0:
                log('Saving audio and alignment...')
                _, lin, al = model.forward_targets(batch["inputs"][:1], batch["input_lengths"][:1], batch["speaker_id"][:1], batch["mel_targets"][:1],
                                                   teacher_forced=True)
                _save_outputs(model, hp, model_dir, "train", step, lin, al)
                _test_losses(model, test_batch)
                _save_outputs(model, hp, model_dir, "test", step, model.linear_outputs, model.alignments)
                log('Test finished for step {}.'.format(step))
    finally:
        batches.close()
    return {"model_dir": model_dir, "step": step, "loss": loss, "losses": losses, "trainer": trainer}


if __name__ == '__main__':
    main()
