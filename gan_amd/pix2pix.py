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
from .diffaug import DiffAugment, parse_policies
from .preprocess import MAX_GRID, MAX_SIGMA, Preprocess, parse_stages
from .quality import QualityMeter, image_quality, summary
from .steps import Pix2PixStep
from .runner import (RESUME_SLOTS, add_common_flags, add_prediction_flags, check_common_flags, check_prediction_flags, drive, finite_lists,
                     save_panels, tile_overlap_of)
from .utils import pix2pix_losses


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


MSSSIM_POWER = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def _msssim_eager(a, b, power=MSSSIM_POWER):
    """1 - mean MS-SSIM(a, b) of two NHWC batches in [-1, 1]: the eager torch restatement of gan_msssim (DESIGN.md section 24;
    tf.image.ssim_multiscale on the display range with max_val 1): per level the map means of cs (of lum * cs on the last), the
    next level the 2 x 2 mean with the last row / column repeated where a side is odd, the product of the clamped means raised to
    `power` per image and channel; differentiable through autograd."""
    ua, ub = (0.5 * t.float().permute(0, 3, 1, 2) + 0.5 for t in (a, b))
    c = ua.shape[1]
    k = torch.arange(11, dtype=torch.float64, device=ua.device) - 5
    g = torch.exp(-k * k / (2 * 1.5 ** 2))
    g = (g / g.sum()).float()
    win = (g[:, None] * g[None, :]).expand(c, 1, 11, 11).contiguous()
    F = lambda t: torch.nn.functional.conv2d(t, win, groups=c)
    pool = lambda t: torch.nn.functional.avg_pool2d(torch.nn.functional.pad(t, (0, t.shape[3] % 2, 0, t.shape[2] % 2), mode='replicate'), 2)
    ms = None
    for j, w in enumerate(power):
        mx, my = F(ua), F(ub)
        term = (2 * (F(ua * ub) - mx * my) + 9e-4) / (F(ua * ua + ub * ub) - mx * mx - my * my + 9e-4)
        if j == len(power) - 1:
            term = term * (2 * mx * my + 1e-4) / (mx * mx + my * my + 1e-4)
        m = term.mean(dim=(2, 3))
        pos = m > 0                  # the clamped region has gradient 0 by definition
        f = torch.where(pos, torch.where(pos, m, torch.ones_like(m)) ** w, torch.zeros_like(m))
        ms = f if ms is None else ms * f
        if j + 1 < len(power):
            ua, ub = pool(ua), pool(ub)
    return 1.0 - ms.mean(dim=1).mean()


def _edge_eager(a, b):
    """The Sobel edge term of two NHWC batches: the eager torch restatement of gan_edge_l1 - the mean of
    (|Sx * d| + |Sy * d|) / 16 over the valid positions of d = a - b, differentiable through autograd."""
    d = (a.float() - b.float()).permute(0, 3, 1, 2)
    c = d.shape[1]
    sx = torch.tensor([[-1., 0., 1.], [-2., 0., 2.], [-1., 0., 1.]], device=d.device)
    win = lambda k: k.expand(c, 1, 3, 3).contiguous()
    ex = torch.nn.functional.conv2d(d, win(sx), groups=c)          # (conv2d correlates, as the definition does)
    ey = torch.nn.functional.conv2d(d, win(sx.t()), groups=c)
    return (ex.abs() + ey.abs()).mean() / 16.0


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
        (self.generator_ema,) = self._init_trainer(averaged=(self.generator,))
        self._preprocessors = None
        self.diffaug = None        # --diffaugment: one DiffAugment for the training steps of every batch size (built with the first of them)

    def networks(self):
        return (self.generator, self.discriminator)

    # ---- input pipeline (pix2pix.py:34-165) ------------------------------------------------------
    def preprocessors(self):
        """(input half, target half): the Preprocess of --preprocess-input / --preprocess-target; both empty
        without the flags."""
        if self._preprocessors is None:
            cfg = self.config
            kw = dict(clip=float(cfg.get('clahe_clip', 1.0)), grid=int(cfg.get('clahe_grid', 15)), sigma=float(cfg.get('blur_sigma', 0.5)))
            self._preprocessors = tuple(Preprocess(cfg.get(k) or '', **kw) for k in ('preprocess_input', 'preprocess_target'))
        return self._preprocessors

    def preprocess_pair(self, img):
        """The decoded uint8 pair with each half run through its Preprocess, a half being a region of its own (the very bytes
        DeviceDataset(preprocess_a=, preprocess_b=) leaves in the resident buffer); the image itself without the flags."""
        pa, pb = self.preprocessors()
        if not pa and not pb:
            return img
        H, W = img.shape[:2]
        first, second = (0, 0, H, W // 2), (0, W // 2, H, W - W // 2)
        ra, rb = (first, second) if self.config['input_img_orient'] == 'left' else (second, first)
        for pre, region in ((pa, ra), (pb, rb)):
            if pre:
                img = pre.apply_host(img, [region])
        return img

    def split_img(self, image_file: str):
        pa, pb = self.preprocessors()
        if not pa and not pb:
            return D.split_img(super().load(image_file, resize=False), self.config['input_img_orient'])
        img = self.preprocess_pair(D.decode(image_file, int(self.config['channels'])))       # uint8, before the cast of `load`
        return D.split_img(img.astype(np.float32), self.config['input_img_orient'])

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
            pa, pb = self.preprocessors()
            ds = lambda files, jitter: D.DeviceDataset(full(files), int(self.config['channels']), self.config['img_size'], dev, 'pair',
                                                       jitter, self.config['input_img_orient'], cap, preprocess_a=pa, preprocess_b=pb)
            return (D.DeviceBatches(ds(train, True), bs, lambda: D.draw_jitter(self._rng), make_example=self.process_images_train),
                    D.DeviceBatches(ds(val, False), bs, make_example=self.process_images_pred),
                    D.DeviceBatches(ds(test, False), bs, make_example=self.process_images_pred))
        return (D.Batches(full(train), self.process_images_train, bs, dev),
                D.Batches(full(val), self.process_images_pred, bs, dev),
                D.Batches(full(test), self.process_images_pred, bs, dev))

    # ---- losses / step (pix2pix.py:167-218) ------------------------------------------------------
    def generator_loss(self, disc_generated_output, gen_output, target, input_image):
        gan_loss = self.loss_obj(1.0, disc_generated_output)
        kind = str(self.config['generator_loss']).replace('-', '_')
        assert kind in ('l1', 'dssim', 'msssim', 'msssim_l1'), \
            "the secondary generator loss is 'l1', 'dssim', 'msssim' or 'msssim-l1' ('ssim' is refused by parse_opt)"
        target = torch.as_tensor(target, device=self.ctx.device).float()
        if kind == 'dssim':
            gan_loss2 = _dssim_eager(gen_output, target)
        elif kind == 'msssim':
            gan_loss2 = _msssim_eager(gen_output, target)
        elif kind == 'msssim_l1':       # Zhao et al. 2017: (1 - alpha) L1 + alpha (1 - MS-SSIM)
            alpha = float(self.config.get('msssim_alpha') or 0.84)
            gan_loss2 = (1.0 - alpha) * (target - gen_output).abs().mean() + alpha * _msssim_eager(gen_output, target)
        else:
            gan_loss2 = (target - gen_output).abs().mean()
        edge_weight = float(self.config.get('edge_weight') or 0.0)
        if edge_weight > 0.0:               # --edge-weight: a second term in the secondary slot
            gan_loss2 = gan_loss2 + edge_weight * _edge_eager(gen_output, target)
        return gan_loss + (self.config['lambda'] * gan_loss2), gan_loss, gan_loss2

    def _diffaug_for(self, training):
        """config['diffaugment']: the augmentation of what the discriminator sees in training steps; the
        model owns the table and the draw counter, as it owns a pool - a last partial batch continues the same sequence."""
        policies = parse_policies(self.config.get('diffaugment') or '')
        if not training or not policies:
            return None
        if self.diffaug is None:
            self.diffaug = DiffAugment(self.ctx, policies, seed=int(self.config.get('seed', 123)))
        return self.diffaug

    def _build_step(self, batch, training):
        return Pix2PixStep(self.ctx, batch, self.config['img_size'], int(self.config['channels']), lam=self.config['lambda'],
                           lr=self.config['learning_rate'], beta_1=self.config['beta_1'], beta_2=self.config['beta_2'],
                           seed=int(self.config.get('seed', 123)), mask_stream=0 if training else 16, nets=(self.generator.net, self.discriminator.net),
                           generator_loss=str(self.config.get('generator_loss', 'l1')).replace('-', '_'),
                           msssim_alpha=float(self.config.get('msssim_alpha') or 0.84), gan_loss=self.config.get('gan_loss', 'bce'),
                           lr_schedule=self.lr_schedule if training else None, diffaug=self._diffaug_for(training),
                           edge_weight=float(self.config.get('edge_weight') or 0.0))

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
        self.val_quality = {'SSIM': [], 'PSNR': [], 'MAE': []}
        self.val_quality_ema = {'SSIM': [], 'PSNR': [], 'MAE': []}
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
        return self._fit(output_path, checkpoint_manager, pix2pix_losses(), lambda: train_ds, lambda: val_ds, len(train_ds),
                         ('Generator Total Loss', 'Discriminator Loss'),
                         lambda path: self.generate_images(self.generator, example_input[:1], example_target[:1], path), after_epoch,
                         datasets=(train_ds, val_ds, test_ds))

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
        S, c, V = int(self.config['img_size']), int(self.config['channels']), tile_overlap_of(self.config)
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
            img = self.preprocess_pair(img)          # (the widths are even here: the halves are the regions of the training data)
            src = torch.from_numpy(img.copy()).to(self.ctx.device)      # the one upload
            pred = self.generator.infer_tiled(src, tile=S, overlap=V, col0=ci, width=half, fold=False)
            if meter is not None:
                meter.add(image_quality(self.ctx, pred[None], lut[src[:, ct:ct + half].long()][None]))
            host = lambda c0: D.normalize(img[:, c0:c0 + half].astype(np.float32))
            save_panels(os.path.join(plot_path, f"img{k}.png"), [('Input Image', host(ci)), ('Ground Truth', host(ct)),
                                                                 ('Predicted Image', pred.cpu().numpy())], gray=self.config['channels'] == '1')


class Options(argparse.Namespace):
    """The parsed Pix2Pix command line.  --diffaugment, --edge-weight, --msssim-alpha and the preprocessing flags are this driver's own training options: they live in slots beside the flag
    dictionary (vars(opt) stays the set of flags the two drivers are compared on) and reaches the model's config - and
    config.json - through runner.config_of."""
    __slots__ = ('diffaugment', 'edge_weight', 'msssim_alpha', 'preprocess_input', 'preprocess_target', 'clahe_clip', 'clahe_grid',
                 'blur_sigma') + RESUME_SLOTS


def parse_opt(argv=None):
    """Same flags / defaults / assertions as pix2pix.py:341-377 (+ this project's: runner.add_common_flags and the ones below)."""
    argv = sys.argv[1:] if argv is None else argv
    parser = argparse.ArgumentParser()
    parser.add_argument('--data', type=str, help='path to data', required=True)
    add_common_flags(parser, argv, generator='the generator', networks='generator and discriminator')
    parser.add_argument('--generator-loss', type=str, default='l1', choices=['l1', 'ssim', 'dssim', 'msssim', 'msssim-l1'],
                        help="secondary generator loss: 'l1' = mean |target - generated|; 'dssim' = 1 - mean SSIM(generated, target), computed "
                             "with its gradient on the GPU; 'msssim' = 1 - mean MS-SSIM(generated, target) over five scales "
                             "(tf.image.ssim_multiscale's power factors); 'msssim-l1' = (1 - A) * l1 + A * msssim "
                             "with A = --msssim-alpha; 'ssim' (the reference's input-against-target term) is refused")
    parser.add_argument('--msssim-alpha', type=float, default=None,
                        help="mixing weight A of --generator-loss msssim-l1, 0 < A <= 1 (default 0.84, Zhao et al. 2017); refused with any "
                             "other loss")
    parser.add_argument('--diffaugment', type=str, default='',
                        help="differentiable augmentation of everything the discriminator sees in training steps (Zhao et al. 2020), "
                             "for small datasets: a comma-separated subset of translation,cutout,brightness,saturation; default: none "
                             "(the reference)")
    parser.add_argument('--edge-weight', type=float, default=0.0,
                        help="weight W of a Sobel edge term added to the secondary generator loss, relative to --lambda: the generator "
                             "minimises gan + lambda * (secondary + W * mean |Sobel(generated - target)|); default 0: no edge term "
                             "(the reference)")
    stages_help = ("a comma-separated subset of clahe,blur,sharpen, applied in that order to the decoded uint8 {half} half of every pair "
                   "at read-in, on the GPU with --data-cache device: contrast-limited adaptive histogram equalisation (--clahe-clip, "
                   "--clahe-grid), a Gaussian blur (--blur-sigma), a 3 x 3 sharpening filter; the half is a region of its own "
                   "(reflected borders) and every channel of an RGB image is processed as its own plane (per-channel equalisation, "
                   "no colour-space conversion); training, validation, test and --predict all see the same bytes; default: none")
    parser.add_argument('--preprocess-input', type=str, default='', metavar='STAGES', help=stages_help.format(half='input'))
    parser.add_argument('--preprocess-target', type=str, default='', metavar='STAGES', help=stages_help.format(half='target'))
    parser.add_argument('--clahe-clip', type=float, default=1.0, help="CLAHE clip limit as cv2.createCLAHE's clipLimit, >= 0 (0: no clipping); default 1.0")
    parser.add_argument('--clahe-grid', type=int, default=15, help=f"CLAHE tiles per side (tileGridSize), 1 .. {MAX_GRID}; default 15")
    parser.add_argument('--blur-sigma', type=float, default=0.5, help=f"sigma of the blur stage, 0 < sigma <= {MAX_SIGMA}; default 0.5")
    parser.add_argument('--input-img-orient', type=str, default='left', choices=['left', 'right'], help='whether input image is on left (i.e. target right) or vice-versa')
    parser.add_argument('--lambda', type=int, default=100, help='lambda value for secondary generator loss (L1 / dSSIM)')
    add_prediction_flags(parser, image='half', resized=' (the reference)',
                         metrics="image quality of the generator against the ground truth (SSIM as tf.image.ssim, PSNR, MAE), computed on "
                                 "the GPU: --train writes logs/val_quality.json (per epoch) and logs/test_quality.json, --predict "
                                 "writes logs/prediction_metrics.json")
    args = parser.parse_args(argv, namespace=Options())
    if args.generator_loss == 'ssim':
        # pix2pix.py:182-184 computes tf.image.ssim(input_image, target): no gradient reaches the generator and the total becomes
        # a (batch,) vector.  That degenerate term is not built here, and training silently with L1
        # under an 'ssim' label would not be a drop-in: refuse.
        parser.error("--generator-loss ssim is not supported by gan_amd (the reference's SSIM term compares input with target and "
                     "carries no gradient, pix2pix.py:182-184); use the default --generator-loss l1, or --generator-loss dssim "
                     "for 1 - SSIM(generated, target)")
    if args.msssim_alpha is not None and args.generator_loss != 'msssim-l1':
        parser.error(f"--msssim-alpha belongs to --generator-loss msssim-l1, not to --generator-loss {args.generator_loss}")
    if args.msssim_alpha is None:
        args.msssim_alpha = 0.84
    if not 0.0 < args.msssim_alpha <= 1.0:
        parser.error(f"--msssim-alpha {args.msssim_alpha} must be a weight in (0, 1]")
    if not args.edge_weight >= 0.0 or args.edge_weight == float('inf'):
        parser.error(f"--edge-weight {args.edge_weight} must be a finite weight >= 0")
    for flag in ('preprocess_input', 'preprocess_target'):
        try:
            setattr(args, flag, ','.join(parse_stages(getattr(args, flag))))       # (canonical order: what config.json records)
        except ValueError as e:
            parser.error(f"--{flag.replace('_', '-')}: {e}")
    try:
        Preprocess((), args.clahe_clip, args.clahe_grid, args.blur_sigma)
    except ValueError as e:
        parser.error(f"--clahe-clip / --clahe-grid / --blur-sigma: {e}")
    try:
        args.diffaugment = ','.join(parse_policies(args.diffaugment))        # (canonical order: what config.json records)
    except ValueError as e:
        parser.error(f"--diffaugment: {e}")
    check_common_flags(parser, args)
    check_prediction_flags(parser, args)
    return args


def _write_quality_logs(p2p, run, test):
    """--quality-metrics true: the per-epoch validation metrics and those of the test set, also on the averaged weights."""
    if str(p2p.config.get('quality_metrics', 'false')) != 'true':
        return
    run.write_json('val_quality.json', finite_lists(p2p.val_quality))
    run.write_json('test_quality.json', summary(p2p.evaluate(test)))
    if p2p._ema_active():
        run.write_json('val_quality_ema.json', finite_lists(p2p.val_quality_ema))
        with p2p.generator_ema.averaged():
            run.write_json('test_quality_ema.json', summary(p2p.evaluate(test)))


def main(opt):
    """`python pix2pix.py --train ...` on one GPU, or `torchrun --nproc-per-node N pix2pix.py --train ...` for data-parallel
    training (runner.drive)."""
    drive(opt, Pix2Pix, 'Pix2Pix', strict_logs=True, max_to_keep=1, predictor='generator', quality_logs=_write_quality_logs,
          checkpoint_names=('generator_optimizer', 'discriminator_optimizer', 'generator', 'discriminator'))


if __name__ == '__main__':
    main(parse_opt())
