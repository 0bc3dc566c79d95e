"""Pix2Pix with the reference's surface (pix2pix.py:27-461): class `Pix2Pix(GAN)`, `train_step`, `fit`,
`predict`, `parse_opt`, `main` — same flags, defaults, assertions, run-directory layout and metric keys; the
arithmetic of `train_step` runs as one captured hipGraph of hand-written MI355X kernels (gan_amd/steps.py)."""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

from . import data as D
from . import ddp
from . import tiling
from .base_gan import GAN
from .checkpoint import Checkpoint, CheckpointManager, latest_checkpoint
from .ema import WeightAverage
from .quality import QualityMeter, image_quality, summary
from .steps import Pix2PixStep
from .runner import Run, add_lr_decay_flags, check_lr_decay_flags, lr_schedule_for, plot_loss_curves, run_epochs, save_panels
from .utils import pix2pix_losses


def _step_state(ctx, st):
    """Device state a warm-up pass of capture() advances besides weights and Adam moments: the fp16 loss-scale state and the
    per-call dropout draw counters (every new batch size captures a new step: without this each capture would move them)."""
    ts = [ctx.ls] if ctx.ls is not None else []
    ts += [net.params.lr_now for net in st.nets() if net.params.lr_now is not None]       # (the rate a scheduled update reports)
    for call in vars(st).values():
        md = getattr(call, 'mask_draws', None)
        if isinstance(md, torch.Tensor):
            ts.append(md)
    return [(t, t.clone()) for t in ts]


def _restore_step_state(saved):
    for t, v in saved:
        t.copy_(v)


def _dssim_eager(a, b):
    """1 - mean SSIM(a, b) of two NHWC batches in [-1, 1]: the eager torch restatement of gan_dssim (DESIGN.md section 14;
    tf.image.ssim on the display range 0.5 * x + 0.5 with max_val 1), differentiable through autograd."""
    ua, ub = (0.5 * t.float().permute(0, 3, 1, 2) + 0.5 for t in (a, b))
    c = ua.shape[1]
    k = torch.arange(11, dtype=torch.float64, device=ua.device) - 5
    g = torch.exp(-k * k / (2 * 1.5 ** 2))
    g = (g / g.sum()).float()
    win = (g[:, None] * g[None, :]).expand(c, 1, 11, 11).contiguous()
    F = lambda t: torch.nn.functional.conv2d(t, win, groups=c)
    mx, my = F(ua), F(ub)
    lum = (2 * mx * my + 1e-4) / (mx * mx + my * my + 1e-4)
    cs = (2 * (F(ua * ub) - mx * my) + 9e-4) / (F(ua * ua + ub * ub) - mx * mx - my * my + 9e-4)
    return 1.0 - (lum * cs).mean()


class Pix2Pix(GAN):
    def __init__(self, config):
        super().__init__(config)
        c = int(self.config['channels'])
        seed = int(self.config.get('seed', 123))
        self.generator = super().Generator(shape=(self.config['img_size'], self.config['img_size'], c), seed=seed)
        self.discriminator = super().Discriminator(target=True, seed=seed + 1)
        mk = lambda: super(Pix2Pix, self).optimizer(learning_rate=self.config['learning_rate'], beta_1=self.config['beta_1'],
                                                   beta_2=self.config['beta_2'])
        self.generator_optimizer = mk().bind(self.generator.net.params)
        self.discriminator_optimizer = mk().bind(self.discriminator.net.params)
        self._steps = {}          # (batch, training) -> (Pix2PixStep, graph replay)
        self.dist = ddp.DistInfo(0, 1, self.config.get('device'))      # main() replaces it in a data-parallel run
        self._rng = np.random.default_rng(seed)
        self.sync = None          # gan_amd.ddp.GradSync for data-parallel training
        self.lr_schedule = None   # nets.LrSchedule of the training steps: fit() derives it from the config
        self.learning_rates = []  # ... and notes the generator's rate at the end of every epoch
        # moving average of the generator weights: every replayed training step moves it
        self.generator_ema = None
        ema_decay = float(self.config.get('ema_decay', 0.0))
        if ema_decay > 0 or str(self.config.get('predict_weights', 'raw')) == 'ema':
            self.generator_ema = WeightAverage(self.generator, ema_decay, str(self.config.get('ema_warmup', 'true')) == 'true')

    def enable_data_parallel(self, info, wire='bf16', exchange='allreduce'):
        """One process per GPU (torchrun): gradients are averaged over the ranks with RCCL all-reduces overlapped with the
        backward pass (gan_amd/steps.py bucketed schedule); BatchNorm statistics stay per replica; the augmentation stream and
        the dropout masks differ per rank.  The reference is single-device (base_gan.py:18-19 only prints the GPU count)."""
        self.dist = info
        if info.world > 1:
            self._rng = np.random.default_rng(int(self.config.get('seed', 123)) + 7919 * info.rank)
            self.sync = ddp.GradSync([self.generator.net.params.grad, self.discriminator.net.params.grad],
                                     compress_bf16=(wire == 'bf16'), lib=self.ctx.lib, exchange=exchange)

    # ---- input pipeline (pix2pix.py:34-165) ------------------------------------------------------
    def split_img(self, image_file: str):
        return D.split_img(super().load(image_file, resize=False), self.config['input_img_orient'])

    def random_crop(self, input_image, real_image, height: int, width: int):
        y, x = self._rng.integers(0, input_image.shape[0] - height + 1), self._rng.integers(0, input_image.shape[1] - width + 1)
        return input_image[y:y + height, x:x + width], real_image[y:y + height, x:x + width]

    def random_jitter(self, input_image, real_image):
        return D.random_jitter_pair(input_image, real_image, self.config['img_size'], self._rng)

    def process_images_train(self, image_file: str):
        a, b = self.split_img(image_file)
        a, b = self.random_jitter(a, b)
        return super().normalize(a), super().normalize(b)

    def process_images_pred(self, image_file: str):
        a, b = self.split_img(image_file)
        s = self.config['img_size']
        return super().normalize(super().resize(a, s, s)), super().normalize(super().resize(b, s, s))

    def image_pipeline(self, predict: bool = False):
        print("\nReading in and processing images.\n", flush=True)
        contents = [i for i in os.listdir(self.config['data']) if 'png' in i or 'jpg' in i]
        assert contents, "No images found in data directory!"
        full = lambda names: [self.config['data'] + '/' + i for i in names]
        dev = self.ctx.device
        if predict:
            return D.Batches(full(contents), self.process_images_pred, 1, None), None, None
        train, val, test = D.pix2pix_split(contents, self.config['seed'], self.config['test_img'], self.config['validation_size'])
        train, val = (ddp.shard_files(f, self.dist.rank, self.dist.world) for f in (train, val))     # (every rank made the same split)
        bs = self.config["batch_size"]
        if self.config.get('data_cache', 'host') == 'device':        # decoded once, augmented by gan_augment_u8
            cap = int(float(self.config.get('data_cache_gb', 64)) * 2**30)
            ds = lambda files, jitter: D.DeviceDataset(full(files), int(self.config['channels']), self.config['img_size'], dev, 'pair',
                                                       jitter, self.config['input_img_orient'], cap)
            return (D.DeviceBatches(ds(train, True), bs, lambda: D.draw_jitter(self._rng), make_example=self.process_images_train),
                    D.DeviceBatches(ds(val, False), bs, make_example=self.process_images_pred),
                    D.DeviceBatches(ds(test, False), bs, make_example=self.process_images_pred))
        return (D.Batches(full(train), self.process_images_train, bs, dev),
                D.Batches(full(val), self.process_images_pred, bs, dev),
                D.Batches(full(test), self.process_images_pred, bs, dev))

    # ---- losses / step (pix2pix.py:167-218) ------------------------------------------------------
    def generator_loss(self, disc_generated_output, gen_output, target, input_image):
        gan_loss = self.loss_obj(1.0, disc_generated_output)
        kind = self.config['generator_loss']
        assert kind in ('l1', 'dssim'), "the secondary generator loss is 'l1' or 'dssim' ('ssim' is refused by parse_opt)"
        target = torch.as_tensor(target, device=self.ctx.device).float()
        gan_loss2 = _dssim_eager(gen_output, target) if kind == 'dssim' else (target - gen_output).abs().mean()
        return gan_loss + (self.config['lambda'] * gan_loss2), gan_loss, gan_loss2

    def _step_for(self, batch, training):
        key = (batch, bool(training))
        if key not in self._steps:
            st = Pix2PixStep(self.ctx, batch, self.config['img_size'], int(self.config['channels']), lam=self.config['lambda'],
                             lr=self.config['learning_rate'], beta_1=self.config['beta_1'], beta_2=self.config['beta_2'],
                             seed=int(self.config.get('seed', 123)), mask_stream=0 if training else 16, nets=(self.generator.net, self.discriminator.net),
                             generator_loss=self.config.get('generator_loss', 'l1'), gan_loss=self.config.get('gan_loss', 'bce'),
                             lr_schedule=self.lr_schedule if training else None)
            st.sync = self.sync
            if training and self.generator_ema is not None:
                st.ema = (self.generator_ema,)
            saved = self._snapshot()       # capture() runs warm-up passes (they also move BatchNorm's moving statistics): undo them
            extra = _step_state(self.ctx, st)
            replay = st.capture(training=training)
            self._restore(saved)
            _restore_step_state(extra)
            self._steps[key] = (st, replay)
        return self._steps[key]

    def _ema_active(self):
        return self.generator_ema is not None and self.generator_ema.decay > 0

    def _snapshot(self):
        return [(ps, ps.master.clone(), ps.m.clone(), ps.v.clone(), ps.step.clone(), {k: v.clone() for k, v in ps.state.items()})
                for ps in (self.generator.net.params, self.discriminator.net.params)]

    def _restore(self, saved):
        for ps, w, m, v, step, state in saved:
            ps.master.copy_(w); ps.m.copy_(m); ps.v.copy_(v); ps.step.copy_(step)
            for k, t in state.items():
                ps.state[k].copy_(t)
            ps.prepare()

    def train_step(self, input_image, target, training: bool = True):
        """-> (gen_total_loss, gen_gan_loss, gen_gan_loss2, disc_loss) as 0-d device tensors (no host sync)."""
        x = torch.as_tensor(input_image).to(self.ctx.device, torch.float32)
        y = torch.as_tensor(target).to(self.ctx.device, torch.float32)
        st, replay = self._step_for(x.shape[0], training)
        losses = replay(x.contiguous(), y.contiguous())[:4].clone()
        return losses[0], losses[1], losses[2], losses[3]

    # ---- images / loops (pix2pix.py:220-339) -----------------------------------------------------
    def generate_images(self, model, test_input, tar, path_filename: str, quality=None):
        """Input | ground truth | `model(test_input, training=True)` (batch statistics and dropout on, pix2pix.py:228).
        quality: a QualityMeter that receives the metrics of this very prediction against `tar`."""
        pred = model(test_input, training=True)
        if quality is not None:
            quality.add(image_quality(self.ctx, pred, tar))
        pred = pred.cpu().numpy()
        host = lambda t: np.asarray(torch.as_tensor(t).cpu())
        save_panels(path_filename, [('Input Image', host(test_input)[0]), ('Ground Truth', host(tar)[0]), ('Predicted Image', pred[0])],
                    gray=self.config['channels'] == '1')

    def _evaluate_into(self, meter, ds, training=False):
        """Enqueue the predictions and the metrics of every batch of `ds` (no host sync)."""
        if training:            # the reference's batch-1 generator(x, training=True): batch statistics, dropout
            for x, y in ds:
                x, y = torch.as_tensor(x), torch.as_tensor(y)
                for k in range(x.shape[0]):
                    meter.add(image_quality(self.ctx, self.generator(x[k:k + 1], training=True), y[k:k + 1]))
            return
        self.generator.fold()   # once: the weights stand still during the pass
        for x, y in ds:
            call = self.generator.infer_call(x, fold=False)
            meter.add(image_quality(self.ctx, call.out_view(), y))      # the typed output view: no unpack

    def evaluate(self, ds, training: bool = False):
        """Image quality of the generator over a dataset of (input, target) batches (gan_amd/quality.py):
        -> {'SSIM': [...], 'PSNR': [...], 'MAE': [...], 'MSE': [...]}, one entry per image in file order.  training=False:
        inference mode, folded once, in the dataset's batches; training=True: the call `generate_images` makes, one image at a
        time.  An inference forward writes no state: training is unchanged by it, bit for bit."""
        meter = QualityMeter()
        self._evaluate_into(meter, ds, training)
        return meter.drain()

    def fit(self, train_ds, val_ds, test_ds, output_path: str, checkpoint_manager=None):
        print("\nTraining...\n", flush=True)
        it = iter(test_ds)
        example_input, example_target = next(it)
        it.close()
        samples = os.path.join(output_path, 'test_images')
        if self.dist.is_main:
            os.makedirs(samples, exist_ok=True)
        save = checkpoint_manager.save if checkpoint_manager is not None else (lambda: None)
        sample = lambda epoch: self.generate_images(self.generator, example_input[:1], example_target[:1],
                                                    os.path.join(samples, f"epoch_{epoch}.png"))
        if not self.dist.is_main:           # rank 0 alone writes checkpoints and sample images
            save = sample = (lambda *a: None)
        self.val_quality = {'SSIM': [], 'PSNR': [], 'MAE': []}
        self.val_quality_ema = {'SSIM': [], 'PSNR': [], 'MAE': []}
        self.lr_schedule = lr_schedule_for(self.config, len(train_ds))      # (before the first training step is built and captured)
        self.learning_rates = []
        after_epoch = None
        if str(self.config.get('quality_metrics', 'false')) == 'true':
            def val_pass(into):         # validation set in inference mode; epoch means over all ranks' images, as the losses
                meter = QualityMeter()
                self._evaluate_into(meter, val_ds)
                mean = ddp.mean_over_ranks(*meter.sums(), self.dist)
                vals = mean.cpu().tolist() if mean is not None else [float('nan')] * 4
                for k, v in zip(into, vals):
                    into[k].append(v)
                return f"val SSIM: {vals[0]:.4f}, PSNR: {vals[1]:.2f} dB, MAE: {vals[2]:.4f}"

            def after_epoch(epoch):
                line = val_pass(self.val_quality)
                if self._ema_active():  # the same pass on the averaged weights
                    with self.generator_ema.averaged():
                        line += " | averaged weights: " + val_pass(self.val_quality_ema)
                return line
        if self.lr_schedule is not None:
            quality_lines = after_epoch

            def after_epoch(epoch):         # the rate of the epoch's last update, read back from the device: one 4-byte copy
                lr = next(st for (_, tr), (st, _) in self._steps.items() if tr).current_lr()
                self.learning_rates.append(lr)
                line = quality_lines(epoch) if quality_lines is not None else None
                return f"learning rate: {lr:.3e}" + (f"\n{line}" if line else "")
        return run_epochs(self.config['epochs'], list(pix2pix_losses()), lambda: train_ds, lambda: val_ds, self.train_step,
                          save, sample, ('Generator Total Loss', 'Discriminator Loss'),
                          epoch_mean=lambda acc, n: ddp.mean_over_ranks(acc, n, self.dist),
                          after_pass=(self.ctx.assert_no_stack_timeout if self.ctx.use_stacks else None), after_epoch=after_epoch)

    def predict(self, predict_ds, output_path: str):
        """config['predict_training'] 'true' (default): the reference's batch-1 `generator(x, training=True)` per image.  'false':
        inference mode (moving statistics, no dropout), folded once - the weights stay fixed while predicting - and run in batches
        of config['batch_size'] images; the same files in the same order.
        config['predict_resolution'] 'native' (inference mode only): every half at its source size, tiled (_predict_native).
        config['quality_metrics'] 'true': -> the image-quality metrics of the very predictions that are written as images, per
        image in file order (Pix2Pix.evaluate's layout); otherwise None."""
        plot_path = os.path.join(output_path, 'prediction_images')
        os.makedirs(plot_path, exist_ok=False)
        meter = QualityMeter() if str(self.config.get('quality_metrics', 'false')) == 'true' else None
        if str(self.config.get('predict_resolution', 'resized')) == 'native':
            self._predict_native(predict_ds.files, plot_path, meter)
            return meter.drain() if meter is not None else None
        if str(self.config.get('predict_training', 'true')) == 'true':
            for k, (inp, tar) in enumerate(predict_ds.unbatch()):
                self.generate_images(self.generator, inp[None], tar[None], os.path.join(plot_path, f"img{k}.png"), quality=meter)
            return meter.drain() if meter is not None else None
        self.generator.fold()
        k = 0
        for chunk in D.chunked(predict_ds.unbatch(), int(self.config['batch_size'])):
            pred = self.generator.infer(np.stack([inp for inp, _ in chunk]), fold=False)
            if meter is not None:
                meter.add(image_quality(self.ctx, pred, np.stack([tar for _, tar in chunk])))
            pred = pred.cpu().numpy()
            for (inp, tar), p in zip(chunk, pred):
                save_panels(os.path.join(plot_path, f"img{k}.png"), [('Input Image', inp), ('Ground Truth', tar), ('Predicted Image', p)],
                            gray=self.config['channels'] == '1')
                k += 1
        return meter.drain() if meter is not None else None

    def _predict_native(self, files, plot_path, meter):
        """Prediction at the source resolution: each file is decoded once and uploaded once as uint8, input
        and target are its two halves by column offset, the input goes through the generator as overlapping img_size tiles
        (GeneratorModel.infer_tiled) and the three panels are written at the source size.  The metrics compare the full-resolution
        prediction with the full-resolution normalised target."""
        S, c = int(self.config['img_size']), int(self.config['channels'])
        V = self.config.get('tile_overlap')
        V = S // 4 if V is None else int(V)
        lut = tiling.normalize_lut(self.ctx)
        self.generator.fold()           # once: the weights stand still while predicting
        for k, f in enumerate(files):
            img = D.decode(f, c)
            H, W = img.shape[:2]
            half = W // 2
            if W % 2:
                raise ValueError(f"{f}: a pair of odd width {W} has halves of different sizes; --predict-resolution native "
                                 "compares the halves pixel by pixel and does not resize")
            if H < S or half < S:
                raise ValueError(f"{f}: each half is {H} x {half}, smaller than --img-size {S}; --predict-resolution native does "
                                 "not pad (use --predict-resolution resized)")
            ci, ct = (0, half) if self.config['input_img_orient'] == 'left' else (half, 0)
            src = torch.from_numpy(img.copy()).to(self.ctx.device)      # the one upload
            pred = self.generator.infer_tiled(src, tile=S, overlap=V, col0=ci, width=half, fold=False)
            if meter is not None:
                meter.add(image_quality(self.ctx, pred[None], lut[src[:, ct:ct + half].long()][None]))
            host = lambda c0: D.normalize(img[:, c0:c0 + half].astype(np.float32))
            save_panels(os.path.join(plot_path, f"img{k}.png"), [('Input Image', host(ci)), ('Ground Truth', host(ct)),
                                                                 ('Predicted Image', pred.cpu().numpy())], gray=self.config['channels'] == '1')


def parse_opt(argv=None):
    """Same flags / defaults / assertions as pix2pix.py:341-377 (+ optional --dtype / --device)."""
    argv = sys.argv[1:] if argv is None else argv
    parser = argparse.ArgumentParser()
    parser.add_argument('--data', type=str, help='path to data', required=True)
    parser.add_argument('--output', type=str, help='path to output results', required=True)
    parser.add_argument('--img-size', type=int, default=256, help='image size h,w')
    parser.add_argument('--batch-size', type=int, default=1, help='batch size per replica')
    parser.add_argument('--buffer-size', type=int, default=99999, help='buffer size')
    parser.add_argument('--channels', type=str, default='1', choices=['1', '3'], help='number of color channels to read in and output')
    parser.add_argument('--logging', type=str, default='true', choices=['true', 'false'], help='turn on/off script logging, e.g. for CLI debugging')
    parser.add_argument('--generator-loss', type=str, default='l1', choices=['l1', 'ssim', 'dssim'],
                        help="secondary generator loss: 'l1' = mean |target - generated|; 'dssim' = 1 - mean SSIM(generated, target), computed "
                             "with its gradient on the GPU; 'ssim' (the reference's input-against-target term) is refused")
    parser.add_argument('--gan-loss', type=str, default='bce', choices=['bce', 'lsgan'],
                        help="adversarial loss on the discriminator's logits: 'bce' = sigmoid cross-entropy (the reference); "
                             "'lsgan' = least squares, mean((logit - target)^2)")
    parser.add_argument('--input-img-orient', type=str, default='left', choices=['left', 'right'], help='whether input image is on left (i.e. target right) or vice-versa')
    parser.add_argument('--seed', type=int, default=123, help='seed value for random number generator')
    group = parser.add_mutually_exclusive_group(required=True)
    group.add_argument('--train', action='store_true', help='train model using data')
    group.add_argument('--predict', action='store_true', help='use pretrained weights to make predictions on data')
    parser.add_argument('--save-weights', type=str, default='true', choices=['true', 'false'], help='save model checkpoints and weights')
    parser.add_argument('--epochs', type=int, default=5, help='number of epochs to train', required='--train' in argv)
    parser.add_argument('--lambda', type=int, default=100, help='lambda value for secondary generator loss (L1 / dSSIM)')
    parser.add_argument('--validation-size', type=float, default=0.1, help='validation set size as share of number of training images')
    parser.add_argument('--test-img', type=int, default=5, help='number of test images to sample')
    parser.add_argument('--learning-rate', type=float, default=2e-4, help='learning rate for Adam optimizer for generator and discriminator')
    parser.add_argument('--beta-1', type=float, default=0.5, help='exponential decay rate for 1st moment of Adam optimizer for generator and discriminator')
    parser.add_argument('--beta-2', type=float, default=0.999, help='exponential decay rate for 2st moment of Adam optimizer for generator and discriminator')
    parser.add_argument('--weights', type=str, help='path to pretrained model weights for prediction', required='--predict' in argv)
    parser.add_argument('--dtype', type=str, default='bf16', choices=['bf16', 'f16', 'f32'], help='MI355X compute/storage dtype (f32 = exact parity path)')
    parser.add_argument('--predict-training', type=str, default='true', choices=['true', 'false'],
                        help="--predict only: 'true' = the reference's generator(x, training=True) at batch 1 (batch statistics, "
                             "dropout); 'false' = Keras inference mode (moving statistics, no dropout) in batches of --batch-size")
    parser.add_argument('--predict-resolution', type=str, default='resized', choices=['resized', 'native'],
                        help="--predict only: 'resized' = every half resized to --img-size first (the reference); 'native' = predict "
                             "at the source size from overlapping --img-size tiles blended on the GPU (needs --predict-training false)")
    parser.add_argument('--tile-overlap', type=int, default=None,
                        help='--predict-resolution native: pixels neighbouring tiles share, 0 ..= img-size / 2 (default img-size / 4)')
    parser.add_argument('--data-cache', type=str, default='host', choices=['host', 'device'],
                        help="--train: 'host' decodes and augments every image on the CPU in every epoch; 'device' decodes each file once, "
                             "keeps the uint8 images in GPU memory and builds every batch there (identical batches)")
    parser.add_argument('--data-cache-gb', type=float, default=64, help='--data-cache device: most GiB of decoded images to keep per GPU')
    parser.add_argument('--quality-metrics', type=str, default='false', choices=['true', 'false'],
                        help="image quality of the generator against the ground truth (SSIM as tf.image.ssim, PSNR, MAE), computed on "
                             "the GPU: --train writes logs/val_quality.json (per epoch) and logs/test_quality.json, --predict "
                             "writes logs/prediction_metrics.json")
    parser.add_argument('--ema-decay', type=float, default=0.0,
                        help='--train: keep an exponential moving average of the generator weights with this decay, updated on the GPU '
                             'after every step and saved with the checkpoint (0 = off; e.g. 0.999)')
    parser.add_argument('--ema-warmup', type=str, default='true', choices=['true', 'false'],
                        help="--ema-decay: 'true' = decay min(ema-decay, (1 + step) / (10 + step)), so that a young average follows the weights")
    parser.add_argument('--predict-weights', type=str, default='raw', choices=['raw', 'ema'],
                        help="--predict: 'raw' = the checkpoint's generator weights; 'ema' = its averaged weights (a run with --ema-decay)")
    add_lr_decay_flags(parser)
    parser.add_argument('--device', type=str, default='cuda:0')
    parser.add_argument('--dist-backend', type=str, default='nccl', choices=['nccl', 'gloo'],
                        help='under torchrun (one process per GPU): collective backend; nccl = RCCL over xGMI')
    parser.add_argument('--wire', type=str, default='bf16', choices=['bf16', 'f32'], help='gradient all-reduce wire format')
    parser.add_argument('--exchange', type=str, default='allreduce', choices=['allreduce', 'rs_ag'],
                        help='gradient exchange: one all-reduce per bucket, or fp32 reduce-scatter + all-gather in the wire format')
    args = parser.parse_args(argv)
    if args.generator_loss == 'ssim':
        # pix2pix.py:182-184 computes tf.image.ssim(input_image, target): no gradient reaches the generator and the total becomes
        # a (batch,) vector.  That degenerate term is not built here, and training silently with L1
        # under an 'ssim' label would not be a drop-in: refuse.
        parser.error("--generator-loss ssim is not supported by gan_amd (the reference's SSIM term compares input with target and "
                     "carries no gradient, pix2pix.py:182-184); use the default --generator-loss l1, or --generator-loss dssim "
                     "for 1 - SSIM(generated, target)")
    if not 0.0 <= args.ema_decay < 1.0:
        parser.error(f"--ema-decay {args.ema_decay} is outside [0, 1)")
    check_lr_decay_flags(parser, args)
    assert (args.img_size == 256) or (args.img_size == 512), "img-size currently only supported for 256 x 256 or 512 x 512 pixels!"
    if args.tile_overlap is None:
        args.tile_overlap = args.img_size // 4
    if not 0 <= args.tile_overlap <= args.img_size // 2:
        parser.error(f"--tile-overlap {args.tile_overlap} is outside [0, img-size / 2 = {args.img_size // 2}]")
    if args.predict_resolution == 'native' and not (args.predict and args.predict_training == 'false'):
        parser.error("--predict-resolution native requires --predict and --predict-training false: tiles are only meaningful in "
                     "inference mode (batch statistics over the tiles of one image are not the reference's semantics)")
    assert (args.validation_size > 0.0 and args.validation_size <= 0.3), "validation size is a proportion and bounded between 0-0.3!"
    assert (args.test_img >= 1), "test-img is an integer and must be >=1!"
    return args


def main(opt):
    """`python pix2pix.py --train ...` on one GPU, or `torchrun --nproc-per-node N pix2pix.py --train ...` for data-parallel
    training: the process group is joined before the first GPU call, rank r owns cuda:r, the training / validation file lists
    are sharded by rank after the seeded split, and rank 0 alone owns the run directory (logs, checkpoints, figures)."""
    info = ddp.init_from_env(opt.device, opt.dist_backend)
    opt.device = info.device or opt.device
    run = Run(opt.output, log_to_file=opt.logging == 'true' and info.is_main, strict_logs=True, writer=info.is_main)
    try:
        p2p = Pix2Pix(vars(opt))
        if opt.train:
            p2p.enable_data_parallel(info, opt.wire, opt.exchange)
        objects = dict(generator_optimizer=p2p.generator_optimizer, discriminator_optimizer=p2p.discriminator_optimizer,
                       generator=p2p.generator, discriminator=p2p.discriminator)
        if p2p.generator_ema is not None:      # after `generator`: restore runs in this order, and an average that finds no
            objects['generator_ema'] = p2p.generator_ema     # weights of its own starts over from the restored generator
        checkpoint = Checkpoint(**objects)
        run.write_json('config.json', p2p.config)
        if opt.predict:
            if info.is_main:
                dataset, _, _ = p2p.image_pipeline(predict=True)
                checkpoint.restore(latest_checkpoint(opt.weights))
                if opt.predict_weights == 'ema':
                    if not p2p.generator_ema.loaded:
                        raise SystemExit(f"--predict-weights ema: checkpoint holds no averaged weights ({opt.weights}); "
                                         "train with --ema-decay")
                    with p2p.generator_ema.averaged():
                        metrics = p2p.predict(dataset, run.root)
                else:
                    metrics = p2p.predict(dataset, run.root)
                if metrics is not None:
                    run.write_json('prediction_metrics.json', summary(metrics))
        else:
            train, validation, test = p2p.image_pipeline(predict=False)
            manager = (CheckpointManager(checkpoint, os.path.join(run.root, 'training_checkpoints'), max_to_keep=1)
                       if opt.save_weights == 'true' and info.is_main else None)
            train_metrics, val_metrics = p2p.fit(train, validation, test, run.root, checkpoint_manager=manager)
            ddp.assert_replicas_in_sync([p2p.generator.net.params, p2p.discriminator.net.params], info)
            if info.is_main:
                if opt.quality_metrics == 'true':
                    run.write_json('val_quality.json', {k: [v if np.isfinite(v) else None for v in vs] for k, vs in p2p.val_quality.items()})
                    run.write_json('test_quality.json', summary(p2p.evaluate(test)))
                    if p2p._ema_active():
                        run.write_json('val_quality_ema.json', {k: [v if np.isfinite(v) else None for v in vs]
                                                                for k, vs in p2p.val_quality_ema.items()})
                        with p2p.generator_ema.averaged():
                            run.write_json('test_quality_ema.json', summary(p2p.evaluate(test)))
                final = run.dir('final_test_imgs', fresh=True)
                for k, (inp, tar) in enumerate(test.unbatch()):
                    p2p.generate_images(p2p.generator, inp[None], tar[None], os.path.join(final, f"img{k}.png"))
                run.write_json('train_metrics.json', train_metrics)
                run.write_json('val_metrics.json', val_metrics)
                if p2p.lr_schedule is not None:
                    run.write_json('learning_rate.json', p2p.learning_rates)
                plot_loss_curves(train_metrics, val_metrics, 'Pix2Pix', os.path.join(run.root, 'figs'))
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


if __name__ == '__main__':
    main(parse_opt())
