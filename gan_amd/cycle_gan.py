"""CycleGAN with the reference's surface (cycle_gan.py:27-502): class `CycleGAN(GAN)`, `train_step`, `fit`,
`predict`, `parse_opt`, `main`; the 6 generator and 4 discriminator invocations of one `train_step`, their
shared backward and four Adam updates run as one captured hipGraph (gan_amd/steps.py::CycleGANStep)."""
from __future__ import annotations

import argparse
import contextlib
import os
import random
import sys

import numpy as np
import torch

from . import cycle_quality as Q
from . import data as D
from . import ddp
from . import tiling
from .base_gan import GAN
from .pool import STREAM_X, STREAM_Y, ImagePool
from .quality import QualityMeter, summary
from .steps import CycleGANStep
from .runner import (RESUME_SLOTS, add_common_flags, add_prediction_flags, check_common_flags, check_prediction_flags, drive, finite_lists,
                     save_panels, tile_overlap_of)
from .utils import cyclegan_losses


class CycleGAN(GAN):
    def __init__(self, config):
        super().__init__(config)
        c = int(self.config['channels'])
        seed = int(self.config.get('seed', 123))
        n = 'instancenorm'                                                             # cycle_gan.py:30-33
        self.generator_g = super().Generator(norm_type=n, shape=(None, None, c), seed=seed, name='generator_g')
        self.generator_f = super().Generator(norm_type=n, shape=(None, None, c), seed=seed + 1, name='generator_f')
        self.discriminator_x = super().Discriminator(norm_type=n, target=False, seed=seed + 2, name='discriminator_x')
        self.discriminator_y = super().Discriminator(norm_type=n, target=False, seed=seed + 3, name='discriminator_y')
        mk = lambda m: super(CycleGAN, self).optimizer(learning_rate=self.config['learning_rate'], beta_1=self.config['beta_1'],
                                                      beta_2=self.config['beta_2']).bind(m.net.params)
        self.generator_g_optimizer, self.generator_f_optimizer = mk(self.generator_g), mk(self.generator_f)
        self.discriminator_x_optimizer, self.discriminator_y_optimizer = mk(self.discriminator_x), mk(self.discriminator_y)
        self.generator_g_ema, self.generator_f_ema = self._init_trainer(averaged=(self.generator_g, self.generator_f))
        # image history pools of the two discriminators (--pool-size): the model's, shared by its training steps
        self.pools = None
        pool_size = int(self.config.get('pool_size') or 0)
        if pool_size < 0:
            raise ValueError(f"pool_size {pool_size} is negative")
        if pool_size > 0:
            self.pools = tuple(ImagePool(self.ctx, int(self.config['img_size']), c, pool_size, seed, sid) for sid in (STREAM_Y, STREAM_X))

    def networks(self):
        return (self.generator_g, self.generator_f, self.discriminator_x, self.discriminator_y)

    # ---- input pipeline (cycle_gan.py:40-152) ----------------------------------------------------
    def random_crop(self, image, height: int, width: int):
        y, x = self._rng.integers(0, image.shape[0] - height + 1), self._rng.integers(0, image.shape[1] - width + 1)
        return image[y:y + height, x:x + width]

    def random_jitter(self, image):
        return D.random_jitter_single(image, self.config['img_size'], self._rng)

    def process_images_train(self, image_file: str):
        return (super().normalize(self.random_jitter(super().load(image_file, resize=True))),)

    def process_images_pred(self, image_file: str):
        s = self.config['img_size']
        return (super().normalize(super().resize(super().load(image_file, resize=True), s, s)),)

    def image_pipeline(self, predict: bool = False):
        print("\nReading in and processing images.\n", flush=True)
        cx = [i for i in os.listdir(self.config['input_images']) if 'png' in i or 'jpg' in i]
        assert cx, "No images found in input image directory!"
        fx = lambda names: [self.config['input_images'] + '/' + i for i in names]
        if predict:
            return D.Batches(fx(cx), self.process_images_pred, 1, None), None, None, None, None
        cy = [i for i in os.listdir(self.config['target_images']) if 'png' in i or 'jpg' in i]
        assert cy, "No images found in target image directory!"
        fy = lambda names: [self.config['target_images'] + '/' + i for i in names]
        random.seed(self.config['seed'])
        test = random.sample(cx, self.config['test_img'])
        val_obs_X = int(np.ceil((len(cx) - self.config['test_img']) * self.config['validation_size']))
        val_obs_Y = int(np.ceil(len(cy) * self.config['validation_size']))
        val_X = random.sample([i for i in cx if i not in test], val_obs_X)
        val_Y = random.sample([i for i in cy], val_obs_Y)
        train_X = [i for i in cx if i not in test and i not in val_X]
        train_Y = [i for i in cy if i not in val_Y]
        train_X, train_Y, val_X, val_Y = (ddp.shard_files(f, self.dist.rank, self.dist.world) for f in (train_X, train_Y, val_X, val_Y))
        bs, dev, sd = self.config["batch_size"], self.ctx.device, self.config['seed']
        if self.config.get('data_cache', 'host') == 'device':        # decoded once, augmented by gan_augment_u8
            cap = int(float(self.config.get('data_cache_gb', 64)) * 2**30)
            ds = lambda files, jitter: D.DeviceDataset(files, int(self.config['channels']), self.config['img_size'], dev, 'single', jitter,
                                                       cap_bytes=cap)
            draw = lambda: D.draw_jitter(self._rng)      # in the consuming thread, X before Y per batch: reproducible run to run
            return (D.DeviceBatches(ds(fx(train_X), True), bs, draw, sd, self.process_images_train),
                    D.DeviceBatches(ds(fy(train_Y), True), bs, draw, sd + 1, self.process_images_train),
                    D.DeviceBatches(ds(fx(val_X), False), bs, None, sd + 2, self.process_images_pred),
                    D.DeviceBatches(ds(fy(val_Y), False), bs, None, sd + 3, self.process_images_pred),
                    D.DeviceBatches(ds(fx(test), False), bs, None, None, self.process_images_pred))
        return (D.Batches(fx(train_X), self.process_images_train, bs, dev, shuffle_seed=sd),
                D.Batches(fy(train_Y), self.process_images_train, bs, dev, shuffle_seed=sd + 1),
                D.Batches(fx(val_X), self.process_images_pred, bs, dev, shuffle_seed=sd + 2),
                D.Batches(fy(val_Y), self.process_images_pred, bs, dev, shuffle_seed=sd + 3),
                D.Batches(fx(test), self.process_images_pred, bs, dev))

    # ---- losses (cycle_gan.py:154-177) -----------------------------------------------------------
    def generator_loss(self, generated):
        return self.loss_obj(1.0, generated)

    def calc_cycle_loss(self, real_image, cycled_image):
        return (torch.as_tensor(real_image).float() - torch.as_tensor(cycled_image).float()).abs().mean() * self.config['lambda']

    def identity_loss(self, real_image, same_image):
        return self.config['lambda'] * 0.5 * (torch.as_tensor(real_image).float() - torch.as_tensor(same_image).float()).abs().mean()

    # ---- step (cycle_gan.py:206-276) -------------------------------------------------------------
    def _build_step(self, batch, training):
        return CycleGANStep(self.ctx, batch, self.config['img_size'], int(self.config['channels']), lam=self.config['lambda'],
                            lr=self.config['learning_rate'], beta_1=self.config['beta_1'], beta_2=self.config['beta_2'],
                            seed=int(self.config.get('seed', 123)), mask_stream=0 if training else 16, nets=tuple(m.net for m in self.networks()),
                            gan_loss=self.config.get('gan_loss', 'bce'), lr_schedule=self.lr_schedule if training else None,
                            pools=self.pools if training else None)

    def train_step(self, real_x, real_y, training: bool = True):
        """-> the reference's 7 losses (cycle_gan.py:275-276) as 0-d device tensors."""
        x = torch.as_tensor(real_x).to(self.ctx.device, torch.float32).contiguous()
        y = torch.as_tensor(real_y).to(self.ctx.device, torch.float32).contiguous()
        st, replay = self._step_for(x.shape[0], training)
        return tuple(replay(x, y)[:7].clone().unbind(0))

    # ---- images / loops (cycle_gan.py:179-204, 278-376) ------------------------------------------
    def generate_images(self, model, test_input, path_filename: str):
        """Input | `model(test_input, training=True)` (cycle_gan.py:186)."""
        pred = model(test_input, training=True).cpu().numpy()
        save_panels(path_filename, [('Input Image', np.asarray(torch.as_tensor(test_input).cpu())[0]), ('Predicted Image', pred[0])],
                    gray=self.config['channels'] == '1')

    @staticmethod
    def _zipped(ds_x, ds_y):
        """tf.data.Dataset.zip of the two unpaired sets (cycle_gan.py:297): stops at the shorter one; a last partial batch
        on one side is cut to the other's size.  Both iterators are closed, so their decode threads end with the pass."""
        ix, iy = iter(ds_x), iter(ds_y)
        try:
            for (x,), (y,) in zip(ix, iy):
                n = min(x.shape[0], y.shape[0])
                yield x[:n], y[:n]
        finally:
            ix.close(); iy.close()

    def _averaged(self):
        """Both generators on their averaged weights (--ema-decay) for the length of the block."""
        stack = contextlib.ExitStack()
        for avg in self.averages:
            stack.enter_context(avg.averaged())
        return stack

    def _fold(self):
        self.generator_g.fold()
        self.generator_f.fold()

    def _evaluate_into(self, meter, ds_x, ds_y=None):
        """Enqueue the cycles and the metrics of every batch (no host sync).  ds_y: zipped with ds_x as the validation pass is."""
        self._fold()        # once: the weights stand still during the pass
        with D.uncounted_passes(ds_x, ds_y):        # the later epochs draw the orders they draw without this pass
            if ds_y is None:
                for (x,) in ds_x:
                    meter.add(Q.cycle_quality(self, x))
            else:
                for x, y in self._zipped(ds_x, ds_y):
                    meter.add(Q.cycle_quality(self, x, y))

    def evaluate(self, ds_x, ds_y=None):
        """Cycle-consistency quality over a dataset (gan_amd/cycle_quality.py), as Pix2Pix.evaluate:
        -> {'cycle_x_ssim': [...], 'cycle_x_psnr': [...], 'cycle_x_mae': [...], 'identity_x_ssim': [...], ...}, one entry per image
        in the order the sets yield them (file order unless a set shuffles): F(G(x)) and F(x) against x; with ds_y also the cycle_y_* / identity_y_* of G(F(y)) and G(y) against y, over
        the zip of the two sets.  Inference mode, in the datasets' batches.  An inference forward writes no state: training is
        unchanged by it, bit for bit."""
        meter = QualityMeter()
        self._evaluate_into(meter, ds_x, ds_y)
        return meter.drain(Q.keys(Q.GROUPS_X if ds_y is None else Q.GROUPS_X + Q.GROUPS_Y))

    def fit(self, train_X, train_Y, val_X, val_Y, test, output_path: str, checkpoint_manager=None):
        print("\nTraining...\n", flush=True)
        it = iter(test)
        example = next(it)[0]
        it.close()
        names = Q.keys()
        self.val_quality = {k: [] for k in names}
        self.val_quality_ema = {k: [] for k in names}
        after_epoch = None
        if str(self.config.get('quality_metrics', 'false')) == 'true':
            def val_pass(into):         # the zipped validation sets in inference mode; epoch means over all ranks' images, as the losses
                meter = QualityMeter()
                self._evaluate_into(meter, val_X, val_Y)
                mean = ddp.mean_over_ranks(*meter.sums(), self.dist)
                vals = mean.cpu().tolist() if mean is not None else [float('nan')] * len(names)
                for k, v in zip(names, vals):
                    into[k].append(v)
                v = dict(zip(names, vals))
                return (f"val cycle x SSIM: {v['cycle_x_ssim']:.4f}, PSNR: {v['cycle_x_psnr']:.2f} dB, MAE: {v['cycle_x_mae']:.4f}; "
                        f"cycle y SSIM: {v['cycle_y_ssim']:.4f}, PSNR: {v['cycle_y_psnr']:.2f} dB, MAE: {v['cycle_y_mae']:.4f}")

            def after_epoch(epoch):
                line = val_pass(self.val_quality)
                if self._ema_active():  # the same pass on the averaged weights
                    with self._averaged():
                        line += " | averaged weights: " + val_pass(self.val_quality_ema)
                return line
        # (the zip of the two unpaired sets stops at the shorter one: that many updates per epoch)
        return self._fit(output_path, checkpoint_manager, cyclegan_losses(), lambda: self._zipped(train_X, train_Y),
                         lambda: self._zipped(val_X, val_Y), min(len(train_X), len(train_Y)),
                         ('Total X->Y Generator Loss', 'Discriminator Y Loss'),
                         lambda path: self.generate_images(self.generator_g, example[:1], path), after_epoch,
                         datasets=(train_X, train_Y, val_X, val_Y, test))

    def predict(self, predict_ds, output_path: str):
        """As Pix2Pix.predict: config['predict_training'] 'false' runs generator_g in inference mode (InstanceNorm has no
        inference-time state: no dropout is the only difference) in batches of config['batch_size'] images.
        config['predict_resolution'] 'native' (inference mode only): every image at its source size, tiled (_predict_native).
        config['quality_metrics'] 'true' (inference mode only: with dropout the cycle is not a deterministic measurement): -> the
        cycle-consistency metrics per image in file order (cycle_x_* and, at img_size, identity_x_*); otherwise None."""
        plot_path = os.path.join(output_path, 'prediction_images')
        os.makedirs(plot_path)
        metrics = str(self.config.get('quality_metrics', 'false')) == 'true'
        gray = self.config['channels'] == '1'
        if str(self.config.get('predict_training', 'true')) == 'true':
            if metrics or str(self.config.get('predict_resolution', 'resized')) == 'native':
                raise ValueError("quality_metrics / predict_resolution native need predict_training 'false': with dropout the cycle "
                                 "is not a deterministic measurement, and tiles are only meaningful in inference mode")
            for k, (img,) in enumerate(predict_ds.unbatch()):
                self.generate_images(self.generator_g, img[None], os.path.join(plot_path, f"img{k}.png"))
            return None
        meter = QualityMeter() if metrics else None
        self._fold()
        if str(self.config.get('predict_resolution', 'resized')) == 'native':
            self._predict_native(predict_ds.files, plot_path, meter, gray)
            return meter.drain(Q.keys(('cycle_x',))) if metrics else None
        k = 0
        for chunk in D.chunked(predict_ds.unbatch(), int(self.config['batch_size'])):
            x = np.stack([img for (img,) in chunk])
            if metrics:             # the cycle starts with this very prediction: it is read from generator_g's eval call afterwards
                meter.add(Q.cycle_quality(self, x))
                pred = self.generator_g.eval_call(*x.shape[:2]).output_f32().cpu().numpy()
            else:
                pred = self.generator_g.infer(x, fold=False).cpu().numpy()
            for (img,), p in zip(chunk, pred):
                save_panels(os.path.join(plot_path, f"img{k}.png"), [('Input Image', img), ('Predicted Image', p)], gray=gray)
                k += 1
        return meter.drain(Q.keys(Q.GROUPS_X)) if metrics else None

    def _predict_native(self, files, plot_path, meter, gray):
        """Prediction at the source resolution (DESIGN.md sections 13 and 19): each file is decoded once and uploaded once as
        uint8, goes through generator_g as overlapping img_size tiles and the two panels are written at the source size.  With a
        meter the prediction comes from cycle_quality_tiled, which sends it on through generator_f and compares the cycled image
        with the normalised source, all on the device."""
        S, c, V = int(self.config['img_size']), int(self.config['channels']), tile_overlap_of(self.config)
        for k, f in enumerate(files):
            img = D.decode(f, c)
            H, W = img.shape[:2]
            if H < S or W < S:
                raise ValueError(f"{f}: the image is {H} x {W}, smaller than --img-size {S}; --predict-resolution native does "
                                 "not pad (use --predict-resolution resized)")
            src = torch.from_numpy(img.copy()).to(self.ctx.device)      # the one upload
            if meter is not None:
                rows, pred, _ = Q.cycle_quality_tiled(self, src, tile=S, overlap=V)
                meter.add(rows)
            else:
                pred = tiling.infer_tiled(self.generator_g, src, tile=S, overlap=V, fold=False)
            panels = [('Input Image', D.normalize(img.astype(np.float32))), ('Predicted Image', pred.cpu().numpy())]
            save_panels(os.path.join(plot_path, f"img{k}.png"), panels, gray=gray)


class Options(argparse.Namespace):
    """The parsed CycleGAN command line.  --pool-size and the prediction / measurement flags (--quality-metrics,
    --predict-resolution, --tile-overlap) are this driver's own options: they live in slots beside the flag dictionary (vars(opt)
    stays the set of flags the two drivers have in common plus their input paths) and reach the model's config through
    runner.config_of."""
    __slots__ = ('pool_size', 'quality_metrics', 'predict_resolution', 'tile_overlap') + RESUME_SLOTS


def parse_opt(argv=None):
    """Same flags / defaults / assertions as cycle_gan.py:379-414 (+ this project's: runner.add_common_flags)."""
    argv = sys.argv[1:] if argv is None else argv
    parser = argparse.ArgumentParser()
    parser.add_argument('--input-images', type=str, help='path to input images', required=True)
    add_common_flags(parser, argv, generator='the two generators', networks='generators and discriminators')
    parser.add_argument('--target-images', type=str, help='path to target images', required='--train' in argv)
    parser.add_argument('--lambda', type=int, default=10, help='lambda parameter value')
    parser.add_argument('--pool-size', type=int, default=0,
                        help='image history pool per discriminator: it is trained on a random mix of current and earlier generated '
                             'images (Zhu et al. 2017 use 50); 0 = none, the reference\'s behaviour. The pools, state and contents, are '
                             'written to checkpoints with the rest of the training state (--resume)')
    add_prediction_flags(parser, image='image', resized=' (the reference)',
                         metrics="cycle-consistency quality, computed on the GPU in inference mode (SSIM as tf.image.ssim, PSNR, MAE of "
                                 "F(G(x)) and F(x) against x, G(F(y)) and G(y) against y): --train writes logs/val_quality.json (per "
                                 "epoch) and logs/test_quality.json, --predict (needs --predict-training false) writes "
                                 "logs/prediction_metrics.json")
    args = parser.parse_args(argv, namespace=Options())
    check_common_flags(parser, args)
    if args.pool_size < 0:
        parser.error(f"--pool-size {args.pool_size} is negative")
    check_prediction_flags(parser, args)
    if args.quality_metrics == 'true' and args.predict and args.predict_training == 'true':
        parser.error("--quality-metrics true with --predict requires --predict-training false: with --predict-training true the "
                     "generators run with dropout, and the cycle F(G(x)) is then not a deterministic measurement")
    return args


def _write_quality_logs(gan, run, test):
    """--quality-metrics true: the per-epoch validation metrics and those of the test set (X only), also on the averaged weights."""
    if str(gan.config.get('quality_metrics', 'false')) != 'true':
        return
    run.write_json('val_quality.json', finite_lists(gan.val_quality))
    run.write_json('test_quality.json', summary(gan.evaluate(test)))
    if gan._ema_active():
        run.write_json('val_quality_ema.json', finite_lists(gan.val_quality_ema))
        with gan._averaged():
            run.write_json('test_quality_ema.json', summary(gan.evaluate(test)))


def main(opt):
    """One GPU, or `torchrun --nproc-per-node N cycle_gan.py --train ...` (data parallel): runner.drive."""
    names = ('generator_g', 'generator_f', 'discriminator_x', 'discriminator_y')        # object names of cycle_gan.py:437-444
    drive(opt, CycleGAN, 'CycleGAN', strict_logs=False, max_to_keep=3, predictor='generator_g', quality_logs=_write_quality_logs,
          checkpoint_names=names + tuple(n + '_optimizer' for n in names))


if __name__ == '__main__':
    main(parse_opt())
