"""Run-directory, logging, metric-file, figure and epoch-loop plumbing shared by the Pix2Pix and CycleGAN drivers.

What is kept from the reference is the CONTRACT: `<output>/<YYYY-MM-DD-HHhMM>/` with
`logs/{Log.txt,config.json,train_metrics.json,val_metrics.json}`, `training_checkpoints/`, `test_images/epoch_N.png`,
`final_test_imgs/imgK.png`, `prediction_images/imgK.png`, `figs/<Model> <Loss name>.png`, the checkpoint cadence
(every 5th epoch and the last, pix2pix.py:308-317) and the `.` tick per 100 mini-batches.  The code is ours: one
`Run` object owns the directory, one epoch driver serves both models, losses stay on the device and are drained once per
epoch (the reference pulls `.numpy()` on every loss of every step, pix2pix.py:276-279).
"""
from __future__ import annotations

import contextlib
import json
import os
import sys
import time
from datetime import datetime

import numpy as np
import torch

from . import ddp
from .checkpoint import Checkpoint, CheckpointManager, latest_checkpoint
from .train_state import NAME as TRAIN_STATE, check_resume


class Run:
    """One timestamped run directory.  `strict_logs`: Pix2Pix refuses to reuse an existing logs/ directory
    (pix2pix.py:392), CycleGAN does not (cycle_gan.py:428)."""

    def __init__(self, output_root: str, log_to_file: bool, strict_logs: bool, writer: bool = True):
        """writer=False: a non-zero rank of a data-parallel run - it creates nothing on disk (rank 0 alone owns the run
        directory, logs, checkpoints and figures) and keeps its console."""
        self.writer = writer
        self.root = os.path.join(output_root, datetime.now().strftime("%Y-%m-%d-%Hh%M"))
        self.logs = os.path.join(self.root, 'logs')
        self._saved = None
        if not writer:
            return
        os.makedirs(self.root, exist_ok=True)
        os.makedirs(self.logs, exist_ok=not strict_logs)
        if log_to_file:
            self._saved = (sys.stdout, sys.stderr)
            sys.stdout = sys.stderr = open(os.path.join(self.logs, "Log.txt"), "w")

    def dir(self, name: str, fresh: bool = False) -> str:
        d = os.path.join(self.root, name)
        if self.writer:
            os.makedirs(d, exist_ok=not fresh)
        return d

    def write_json(self, name: str, obj) -> None:
        if not self.writer:
            return
        with open(os.path.join(self.logs, name), 'w') as f:
            json.dump(obj, f)

    def close(self) -> None:
        if self._saved is not None:
            log = sys.stdout
            sys.stdout, sys.stderr = self._saved
            log.close()
            self._saved = None


def add_lr_decay_flags(parser) -> None:
    """--lr-decay-epochs / --lr-end-factor of both drivers.  Their defaults are None so that
    check_lr_decay_flags can tell a given flag from an absent one; it fills in 0 and 0.0."""
    parser.add_argument('--lr-decay-epochs', type=int, default=None,
                        help='--train: decay the Adam learning rate linearly over the last N epochs, evaluated on the GPU per step '
                             '(default 0 = constant rate, the reference)')
    parser.add_argument('--lr-end-factor', type=float, default=None,
                        help='--lr-decay-epochs: share of --learning-rate that is left at the end of the run, 0 ..= 1 (default 0.0)')


def check_lr_decay_flags(parser, args) -> None:
    given = [f for f, v in (('--lr-decay-epochs', args.lr_decay_epochs), ('--lr-end-factor', args.lr_end_factor)) if v is not None]
    if given and args.predict:
        parser.error(f"{' / '.join(given)}: the learning-rate schedule belongs to --train, not to --predict")
    if args.lr_decay_epochs is None:
        args.lr_decay_epochs = 0
    if args.lr_end_factor is None:
        args.lr_end_factor = 0.0
    if args.lr_decay_epochs < 0:
        parser.error(f"--lr-decay-epochs {args.lr_decay_epochs} is negative")
    if args.train and args.lr_decay_epochs > args.epochs:
        parser.error(f"--lr-decay-epochs {args.lr_decay_epochs} is more than --epochs {args.epochs}")
    if not 0.0 <= args.lr_end_factor <= 1.0:
        parser.error(f"--lr-end-factor {args.lr_end_factor} is outside [0, 1]")


# --resume / --checkpoint-every are declared for both drivers by add_common_flags, and both option classes keep
# them in slots beside the flag dictionary, as they keep their own training options: vars(opt) stays the set of flags the two
# drivers are compared on, and config_of hands the slots to the model's config.
RESUME_SLOTS = ('resume', 'checkpoint_every')


def add_common_flags(parser, argv, generator: str, networks: str) -> None:
    """The flags both drivers take: the reference's common ones (pix2pix.py:341-377, cycle_gan.py:379-414) and this project's.
    argv: --epochs is required with --train, --weights with --predict.  generator / networks: the model's nouns for the help
    texts ('the generator' / 'the two generators', 'generator and discriminator' / 'generators and discriminators')."""
    parser.add_argument('--output', type=str, help='path to output results', required=True)
    parser.add_argument('--img-size', type=int, default=256, help='image size h,w')
    parser.add_argument('--batch-size', type=int, default=1, help='batch size per replica')
    parser.add_argument('--buffer-size', type=int, default=99999, help='buffer size')
    parser.add_argument('--channels', type=str, default='1', choices=['1', '3'], help='number of color channels to read in and output')
    parser.add_argument('--logging', type=str, default='true', choices=['true', 'false'], help='turn on/off script logging, e.g. for CLI debugging')
    parser.add_argument('--seed', type=int, default=123, help='seed value for random number generator')
    group = parser.add_mutually_exclusive_group(required=True)
    group.add_argument('--train', action='store_true', help='train model using data')
    group.add_argument('--predict', action='store_true', help='use pretrained weights to make predictions on data')
    parser.add_argument('--save-weights', type=str, default='true', choices=['true', 'false'], help='save model checkpoints and weights')
    parser.add_argument('--epochs', type=int, default=5, help='number of epochs to train', required='--train' in argv)
    parser.add_argument('--validation-size', type=float, default=0.1, help='validation set size as share of number of training images')
    parser.add_argument('--test-img', type=int, default=5, help='number of test images to sample')
    parser.add_argument('--learning-rate', type=float, default=2e-4, help=f'learning rate for Adam optimizer for {networks}')
    parser.add_argument('--beta-1', type=float, default=0.5, help=f'exponential decay rate for 1st moment of Adam optimizer for {networks}')
    parser.add_argument('--beta-2', type=float, default=0.999, help=f'exponential decay rate for 2st moment of Adam optimizer for {networks}')
    parser.add_argument('--weights', type=str, help='path to pretrained model weights for prediction', required='--predict' in argv)
    parser.add_argument('--dtype', type=str, default='bf16', choices=['bf16', 'f16', 'f32'], help='MI355X compute/storage dtype (f32 = exact parity path)')
    parser.add_argument('--gan-loss', type=str, default='bce', choices=['bce', 'lsgan'],
                        help="adversarial loss on the discriminator logits: 'bce' = sigmoid cross-entropy (the reference); "
                             "'lsgan' = least squares, mean((logit - target)^2)")
    parser.add_argument('--predict-training', type=str, default='true', choices=['true', 'false'],
                        help="--predict only: 'true' = the reference's generator(x, training=True) at batch 1 (batch statistics, "
                             "dropout); 'false' = Keras inference mode (moving statistics, no dropout) in batches of --batch-size")
    parser.add_argument('--data-cache', type=str, default='host', choices=['host', 'device'],
                        help="--train: 'host' decodes and augments every image on the CPU in every epoch; 'device' decodes each file once, "
                             "keeps the uint8 images in GPU memory and builds every batch there")
    parser.add_argument('--data-cache-gb', type=float, default=64, help='--data-cache device: most GiB of decoded images to keep per GPU')
    parser.add_argument('--ema-decay', type=float, default=0.0,
                        help=f'--train: keep an exponential moving average of the weights of {generator} with this decay, updated on the '
                             'GPU after every step and saved with the checkpoint (0 = off; e.g. 0.999)')
    parser.add_argument('--ema-warmup', type=str, default='true', choices=['true', 'false'],
                        help="--ema-decay: 'true' = decay min(ema-decay, (1 + step) / (10 + step)), so that a young average follows the weights")
    parser.add_argument('--predict-weights', type=str, default='raw', choices=['raw', 'ema'],
                        help="--predict: 'raw' = the checkpoint's generator weights; 'ema' = its averaged weights (a run with --ema-decay)")
    add_lr_decay_flags(parser)
    parser.add_argument('--resume', type=str, default=None, metavar='PATH',
                        help='--train: continue an interrupted run bit for bit from a checkpoint of it: a training_checkpoints directory '
                             '(its latest checkpoint) or a prefix .../ckpt-N. The run writes a new run directory and continues behind the '
                             "checkpoint's epoch; everything that shapes the trajectory must be given as in the interrupted run")
    parser.add_argument('--checkpoint-every', type=int, default=5,
                        help='--train: write a checkpoint (and a sample image) after every N-th epoch and after the last one '
                             '(default 5, the reference)')
    parser.add_argument('--device', type=str, default='cuda:0')
    parser.add_argument('--dist-backend', type=str, default='nccl', choices=['nccl', 'gloo'],
                        help='under torchrun (one process per GPU): collective backend; nccl = RCCL over xGMI')
    parser.add_argument('--wire', type=str, default='bf16', choices=['bf16', 'f32'], help='gradient all-reduce wire format')
    parser.add_argument('--exchange', type=str, default='allreduce', choices=['allreduce', 'rs_ag'],
                        help='gradient exchange: one all-reduce per bucket, or fp32 reduce-scatter + all-gather in the wire format')


def add_prediction_flags(parser, image: str, resized: str, metrics: str) -> None:
    """--predict-resolution / --tile-overlap / --quality-metrics.  Each driver declares them with its own nouns: Pix2Pix among the
    flags of vars(opt), CycleGAN in the slots of its option class.  image: what one input image is ('half' / 'image'); resized:
    the parenthesis after 'resized first'; metrics: the help text of --quality-metrics."""
    parser.add_argument('--predict-resolution', type=str, default='resized', choices=['resized', 'native'],
                        help=f"--predict only: 'resized' = every {image} resized to --img-size first{resized}; 'native' = predict "
                             "at the source size from overlapping --img-size tiles blended on the GPU (needs --predict-training false)")
    parser.add_argument('--tile-overlap', type=int, default=None,
                        help='--predict-resolution native: pixels neighbouring tiles share, 0 ..= img-size / 2 (default img-size / 4)')
    parser.add_argument('--quality-metrics', type=str, default='false', choices=['true', 'false'], help=metrics)


def check_prediction_flags(parser, args) -> None:
    """After check_common_flags: the default and the range of --tile-overlap, and what --predict-resolution native needs."""
    if args.tile_overlap is None:
        args.tile_overlap = args.img_size // 4
    if not 0 <= args.tile_overlap <= args.img_size // 2:
        parser.error(f"--tile-overlap {args.tile_overlap} is outside [0, img-size / 2 = {args.img_size // 2}]")
    if args.predict_resolution == 'native' and not (args.predict and args.predict_training == 'false'):
        parser.error("--predict-resolution native requires --predict and --predict-training false: tiles are only meaningful in "
                     "inference mode (batch statistics over the tiles of one image are not the reference's semantics)")


def tile_overlap_of(config) -> int:
    """config['tile_overlap'], or img_size / 4 for a config that was not built by a parser."""
    V = config.get('tile_overlap')
    return int(config['img_size']) // 4 if V is None else int(V)


def finite_lists(per_epoch: dict) -> dict:
    """{key: [epoch mean, ...]} ready for strict JSON: a non-finite value (the PSNR of an exact match) becomes null."""
    return {k: [v if np.isfinite(v) else None for v in vs] for k, vs in per_epoch.items()}


def check_common_flags(parser, args) -> None:
    if not 0.0 <= args.ema_decay < 1.0:
        parser.error(f"--ema-decay {args.ema_decay} is outside [0, 1)")
    check_lr_decay_flags(parser, args)
    if args.resume is not None and not args.train:
        parser.error("--resume continues a training run: it belongs to --train, not to --predict (which takes --weights)")
    if args.checkpoint_every < 1:
        parser.error(f"--checkpoint-every {args.checkpoint_every} is less than 1")
    assert (args.img_size == 256) or (args.img_size == 512), "img-size currently only supported for 256 x 256 or 512 x 512 pixels!"
    assert (args.validation_size > 0.0 and args.validation_size <= 0.3), "validation size is a proportion and bounded between 0-0.3!"
    assert (args.test_img >= 1), "test-img is an integer and must be >=1!"


def lr_schedule_for(config, steps_per_epoch: int):
    """The LrSchedule of a run's config, or None (--lr-decay-epochs 0: the constant rate, nothing is built): the rate is held for
    the first epochs - N epochs and decays over the updates of the last N.  steps_per_epoch: training batches per epoch of this
    replica (data parallel: the same on every rank, ddp.shard_files)."""
    from .nets import LrSchedule
    n = int(config.get('lr_decay_epochs') or 0)
    if n == 0:
        return None
    epochs = int(config['epochs'])
    if not 0 < n <= epochs:
        raise ValueError(f"lr_decay_epochs {n} is outside [0, epochs = {epochs}]")
    if steps_per_epoch <= 0:
        raise ValueError("the learning-rate schedule needs at least one training batch per epoch")
    return LrSchedule(float(config['learning_rate']), float(config.get('lr_end_factor') or 0.0), (epochs - n) * steps_per_epoch,
                      epochs * steps_per_epoch).validate()


def save_panels(path: str, panels, gray: bool) -> None:
    """Side-by-side image panels [(title, HWC array in [-1, 1])] -> one PNG at dpi 200."""
    import matplotlib
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
    fig, axes = plt.subplots(1, len(panels), figsize=(6 * len(panels) - (3 if len(panels) == 3 else 0), 6), squeeze=False)
    for ax, (title, img) in zip(axes[0], panels):
        img = np.clip(np.asarray(img, dtype=np.float32) * 0.5 + 0.5, 0.0, 1.0)
        ax.imshow(img[..., 0], cmap='gray', vmin=0.0, vmax=1.0) if gray else ax.imshow(img)
        ax.set_title(title)
        ax.set_axis_off()
    fig.tight_layout()
    fig.savefig(path, dpi=200)
    plt.close(fig)


def plot_loss_curves(train: dict, val: dict, model_name: str, out_dir: str) -> None:
    """One figure per loss key: training and validation means by epoch (epochs counted from 1), `<Model> <key>.png`."""
    import matplotlib
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
    os.makedirs(out_dir, exist_ok=True)
    for key, tr in train.items():
        epochs = np.arange(1, len(tr) + 1)
        fig, ax = plt.subplots(figsize=(10, 8), dpi=80)
        ax.plot(epochs, tr, alpha=0.7, label='Training')
        ax.plot(epochs[:len(val[key])], val[key], alpha=0.7, label='Validation')
        ax.set(xlabel='Epoch', ylabel='Loss', title=f'{model_name} {key}')
        ax.legend()
        fig.tight_layout()
        fig.savefig(os.path.join(out_dir, f'{model_name} {key}.png'), dpi=200)
        plt.close(fig)


def run_epochs(epochs: int, keys, train_batches, val_batches, step, on_checkpoint, on_sample, headline, epoch_mean=None, after_pass=None,
               after_epoch=None, checkpoint_every: int = 5, hist=None, resumed_after: int = 0):
    """Epoch driver.  train_batches()/val_batches() yield the positional arguments of `step(*args, training)`, which
    returns the per-step loss tensors (device); `headline` = (train key, val key) printed per epoch.
    epoch_mean(acc, n) -> mean loss vector of a pass (data-parallel runs: over all ranks' steps, gan_amd.ddp.mean_over_ranks).
    after_epoch(epoch) -> None or one more line for the epoch print; runs after the validation pass (image-quality metrics).
    checkpoint_every: a checkpoint after every N-th epoch and after the last one; the sample image of an epoch follows its checkpoint,
    except after the last.  hist: the two history dicts to append to (a resumed run: they hold the epochs before).
    resumed_after: E > 0 continues a run whose state was restored from the checkpoint written after epoch E - behind that
    checkpoint, so with the sample image that followed it (drawing it moves BatchNorm's moving statistics), then epochs E + 1 ...
    Returns (train_cost_functions, val_cost_functions): {key: [epoch mean, ...]}."""
    hist = hist if hist is not None else ({k: [] for k in keys}, {k: [] for k in keys})
    t0 = time.time()
    if 0 < resumed_after < epochs and resumed_after % checkpoint_every == 0:
        on_sample(resumed_after)
    for epoch in range(resumed_after + 1, epochs + 1):
        sums = []
        for batches, training in ((train_batches, True), (val_batches, False)):
            acc, n = None, 0
            for args in batches():
                losses = torch.stack(tuple(step(*args, training)))
                acc = losses if acc is None else acc + losses           # stays on the device: no per-step sync
                n += 1
                if training and n % 100 == 0:
                    print('.', end='', flush=True)
            mean = epoch_mean(acc, n) if epoch_mean is not None else ((acc / n) if n else None)
            sums.append(mean.cpu().tolist() if mean is not None else [float('nan')] * len(keys))      # one drain per pass
            if after_pass is not None:
                after_pass()          # device-side error flags are read where the pass has been drained anyway (layer stacks: grid-barrier timeout)
        for h, means in zip(hist, sums):
            for k, v in zip(keys, means):
                h[k].append(v)
        extra = after_epoch(epoch) if after_epoch is not None else None
        last = epoch == epochs
        if epoch % checkpoint_every == 0 or last:
            on_checkpoint()
            if not last:
                on_sample(epoch)
        print(f'\nCumulative training duration at end of epoch {epoch}: {(time.time() - t0) / 60:.2f} min')
        print(f"Train {headline[0]}: {hist[0][headline[0]][-1]:.2f}, {headline[1]}: {hist[0][headline[1]][-1]:.2f}; "
              f"val {headline[0]}: {hist[1][headline[0]][-1]:.2f}, {headline[1]}: {hist[1][headline[1]][-1]:.2f}"
              + (f"\n{extra}" if extra else "") + "\n", flush=True)
    return hist


def config_of(opt) -> dict:
    """The model's config of a parsed command line.  vars(opt) holds the flags the two drivers are compared on: the common set plus
    each driver's input paths and, for Pix2Pix, its loss and prediction modes.  An option class of a driver may carry further,
    model-specific training options beside them as slots (cycle_gan.Options: pool_size); they reach the model - and config.json -
    through here."""
    own = {k: getattr(opt, k) for k in getattr(type(opt), '__slots__', ())}
    return {**vars(opt), **own}


def drive(opt, model_class, name: str, *, strict_logs: bool, max_to_keep: int, checkpoint_names, predictor: str, quality_logs=None):
    """What `main(opt)` of both drivers does.  One GPU, or under `torchrun --nproc-per-node N` data-parallel training: the process
    group is joined before the first GPU call, rank r owns cuda:r, the training / validation file lists are sharded by rank after the
    seeded split, and rank 0 alone owns the run directory (logs, checkpoints, figures).
    name: the model's name in the figures; checkpoint_names: attributes of the model that make up a checkpoint, in the reference's
    order; predictor: the attribute of the generator that draws the final test images; quality_logs(model, run, test): more
    files under logs/ after training, written before the final images (Pix2Pix's image-quality metrics)."""
    info = ddp.init_from_env(opt.device, opt.dist_backend)
    opt.device = info.device or opt.device
    # --resume is refused before the run directory exists and before anything is built on the GPU (SystemExit, the offending key named)
    try:
        resume_from = check_resume(opt.resume, config_of(opt), info.world) if opt.train and getattr(opt, 'resume', None) else None
    except BaseException:
        ddp.shutdown(info, failed=True)
        raise
    run = Run(opt.output, log_to_file=opt.logging == 'true' and info.is_main, strict_logs=strict_logs, writer=info.is_main)
    try:
        model = model_class(config_of(opt))
        if opt.train:
            model.enable_data_parallel(info, opt.wire, opt.exchange)
        objects = {n: getattr(model, n) for n in checkpoint_names}
        # after the generators: restore runs in this order, and an average that finds no weights of its own starts over from theirs
        objects.update({avg.model.obj_name + '_ema': avg for avg in model.averages})
        objects[TRAIN_STATE] = model.train_state      # what a later --resume continues from
        checkpoint = Checkpoint(**objects)
        if resume_from is not None:
            checkpoint.restore(resume_from)
            print(f"Resuming behind epoch {model.train_state.epoch} of {resume_from}", flush=True)
        run.write_json('config.json', model.config)
        if opt.predict:
            if info.is_main:
                dataset = model.image_pipeline(predict=True)[0]
                checkpoint.restore(latest_checkpoint(opt.weights))
                weights = contextlib.ExitStack()
                if opt.predict_weights == 'ema':
                    if not all(avg.loaded for avg in model.averages):
                        raise SystemExit(f"--predict-weights ema: checkpoint holds no averaged weights ({opt.weights}); "
                                         "train with --ema-decay")
                    for avg in model.averages:      # every averaged generator: CycleGAN's cycle runs on the pair that was averaged together
                        weights.enter_context(avg.averaged())
                with weights:
                    metrics = model.predict(dataset, run.root)
                if metrics is not None:
                    from .quality import summary
                    run.write_json('prediction_metrics.json', summary(metrics))
        else:
            *train_val, test = model.image_pipeline(predict=False)
            manager = (CheckpointManager(checkpoint, os.path.join(run.root, 'training_checkpoints'), max_to_keep=max_to_keep)
                       if opt.save_weights == 'true' and info.is_main else None)
            train_metrics, val_metrics = model.fit(*train_val, test, run.root, checkpoint_manager=manager)
            ddp.assert_replicas_in_sync([m.net.params for m in model.networks()], info)
            if info.is_main:
                if quality_logs is not None:
                    quality_logs(model, run, test)
                final = run.dir('final_test_imgs', fresh=True)
                for k, example in enumerate(test.unbatch()):
                    model.generate_images(getattr(model, predictor), *(a[None] for a in example), os.path.join(final, f"img{k}.png"))
                run.write_json('train_metrics.json', train_metrics)
                run.write_json('val_metrics.json', val_metrics)
                if model.lr_schedule is not None:
                    run.write_json('learning_rate.json', model.learning_rates)
                plot_loss_curves(train_metrics, val_metrics, name, os.path.join(run.root, 'figs'))
                if info.world > 1:
                    print(f"data-parallel run: {info.world} ranks, replicas in sync.")
        print("Done.")
    except BaseException:
        try:
            run.close()
        finally:
            ddp.shutdown(info, failed=True)  # no barrier on the way out of an exception: the peers are inside other collectives
        raise
    run.close()
    ddp.shutdown(info)
