"""Train on the impulse-response tree, the flow of main_training.py: data set -> generators -> model by --name -> Trainer
(optimizer, loss switches, learning rate) -> CheckpointManager -> fit.  One process, one GPU.

    python scripts/train.py --dataset ../datasets room_impulse --rooms LargeMeetingRoom --name unet --out ../results/unet
    python scripts/train.py --synthetic 8 --name vqvae --epochs 3 --lr 1e-4 --out ../results/vqvae       # no data set: 8 random batches
    python scripts/train.py --dataset ../datasets room_impulse --wave-loss 0.1 --wave-loss-norm energy --out ../results/unet_wave

The defaults are main_training.py's (:27-47): target size (144, 160, 2), LargeMeetingRoom, both arrays, debug data set, U-Net,
alpha 0.9, no sigmoid / diff loss, 500 epochs, lr 5e-7 with the exponential decay from epoch 80, batch 16, Adam.  A run continues
from the latest checkpoint in --out when there is one (checkpoints are written every second epoch, :363-364).  The features of
the whole data set live on the device (unet_rir_amd.Dataset); a batch is one kernel launch.  --wave-loss WEIGHT adds the loss on the
reconstructed waveform (unet_rir_amd.WaveLoss), --decay-loss WEIGHT the loss on its energy decay curve (unet_rir_amd.DecayLoss) and
--spectral-loss WEIGHT its multi-resolution STFT loss (unet_rir_amd.SpectralLoss): the data set then keeps the waveforms and the
generators hand them out.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import unet_rir_amd as U


def build_model(a, dev):
    """main_training.py:119-161, constructor arguments included."""
    shape, common = (a.height, a.width, 2), dict(batch_size=a.batch, device=dev, dtype=a.dtype)
    if a.name == "ae":
        return U.Autoencoder(shape, (2, 16), conv_filters=(64, 128, 256, 512), conv_kernels=(3, 3, 3, 3), conv_strides=(2, 2, 2, 2),
                             latent_space_dim=64, n_neurons=32 * 64, name=a.name, **common)
    if a.name == "resae":
        return U.ResAE(shape, (2, 16), conv_filters=(32, 64, 128, 256), conv_kernels=(3, 3, 3, 3), conv_strides=(2, 2, 2, 2),
                       latent_space_dim=32, n_neurons=16 * 64, name=a.name, **common)
    if a.name == "vae":
        return U.VAE(shape, (2, 16), conv_filters=(64, 128, 256, 512), conv_kernels=(3, 3, 3, 3), conv_strides=(2, 2, 2, 2),
                     latent_space_dim=64, n_neurons=32 * 64, name=a.name, **common)
    if a.name == "vqvae":      # main_training.py does not build it: the model of dl_models/vqvae.py's own __main__ block (:522-531)
        return U.VQVAE(shape, (2, 16), conv_filters=(32, 64, 128, 256), conv_kernels=(3, 3, 3, 3), conv_strides=(2, 2, 2, 2),
                       latent_space_dim=16, n_neurons=320, name=a.name, **common)
    if a.name == "aenet":      # dl_models/ae_net.py with its defaults (rir_generation.py:6 imports it; main_training.py has no branch)
        return U.AENet(shape, (2, 16), number_filters_0=a.filters, name="AENet", **common)
    if a.name == "diffunet":   # dl_models/diff_u_net.py with its defaults (rir_generation.py:51-63: the 'unet_diff_full' model); add --diff-loss
        return U.DiffUNet(shape, (2, 16), number_filters_0=a.filters, name="U-Net", **common)
    if a.name == "diffvae":    # the model of dl_models/diff_vae.py's own __main__ block (:476-485); add --diff-loss
        return U.DiffVAE(shape, (2, 16), conv_filters=(32, 64, 128, 256), conv_kernels=(3, 3, 3, 3), conv_strides=(2, 2, 2, 2),
                         latent_space_dim=16, n_neurons=20 * 64, name="Diff_VAE", **common)
    return U.UNet(shape, (2, 16), mode=0, number_filters_0=a.filters, kernels=a.kernels, name="U-Net",
                  resize_factor_0=[a.resize_factor_0] * 2, **common)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dataset", nargs=2, metavar=("DIR", "NAME"), help="the tree is DIR/NAME/Room/ZoneX/...Array/*.wav")
    ap.add_argument("--synthetic", type=int, default=0, metavar="N",
                    help="instead of --dataset: N batches of synthetic_batches per epoch (the same ones every epoch), no validation")
    ap.add_argument("--rooms", nargs="+", default=["LargeMeetingRoom"], help="room names, or All")
    ap.add_argument("--arrays", nargs="+", default=["PlanarMicrophoneArray", "CircularMicrophoneArray"])
    ap.add_argument("--resample", choices=("none", "kaiser_best", "kaiser_fast"), default="none",
                    help="files of --dataset that are not at the data set's rate: none (an error), or converted on the device (librosa's res_type names)")
    ap.add_argument("--no-debug", action="store_true", help="load the whole tree (main_training.py runs with debug = True)")
    ap.add_argument("--extract", action="store_true", help="unpack the zone archives first")
    ap.add_argument("--name", choices=("ae", "resae", "vae", "vqvae", "aenet", "diffunet", "diffvae", "unet"), default="unet")
    ap.add_argument("--filters", type=int, default=32, help="number_filters_0 of the U-Net")
    ap.add_argument("--kernels", type=int, default=3)
    ap.add_argument("--resize-factor-0", type=int, choices=(1, 2), default=1,
                    help="U-Net only: 2 runs the network at half resolution (first convolution stride 2, up-sampling folded into the head)")
    ap.add_argument("--height", type=int, default=144)
    ap.add_argument("--width", type=int, default=160)
    ap.add_argument("--dtype", choices=("f32", "bf16"), default="f32")
    ap.add_argument("--alpha", type=float, default=0.9)
    ap.add_argument("--sigmoid-loss", action="store_true")
    ap.add_argument("--diff-loss", action="store_true")
    ap.add_argument("--beta", type=float, default=0.5)
    ap.add_argument("--wave-loss", type=float, default=None, metavar="WEIGHT",
                    help="add WEIGHT / batch * sum_b E_b / D_b on the reconstructed waveform to the loss (needs --dataset; not for vae / vqvae / diffvae)")
    ap.add_argument("--wave-loss-norm", choices=("mse", "energy"), default="mse",
                    help="D_b: the number of samples (mse) or the target's energy (energy: the squared misalignment ratio)")
    ap.add_argument("--decay-loss", type=float, default=None, metavar="WEIGHT",
                    help="add WEIGHT / batch * sum_b Q_b, the mean squared dB error of the energy decay curve of the reconstructed waveform, "
                         "to the loss (needs --dataset; not for vae / vqvae / diffvae)")
    ap.add_argument("--decay-floor-db", type=float, default=60.0, metavar="DB", help="the decay curves are floored DB below the target's energy")
    ap.add_argument("--spectral-loss", type=float, default=None, metavar="WEIGHT",
                    help="add WEIGHT / batch * sum_b Q_b, the multi-resolution STFT loss (squared spectral convergence + squared log-magnitude "
                         "distance) of the reconstructed waveform, to the loss (needs --dataset; not for vae / vqvae / diffvae)")
    ap.add_argument("--spectral-resolutions", default="128:64:32,512:256:128,1024:512:256", metavar="N:WIN:HOP,...",
                    help="the loss's transforms: n_fft:win_length:hop_length, comma-separated (1 to 8)")
    ap.add_argument("--spectral-floor-db", type=float, default=60.0, metavar="DB",
                    help="the magnitudes are smoothed DB below the power a bin carries with the target's energy spread evenly")
    ap.add_argument("--spectral-method", choices=("dft", "fft"), default="dft",
                    help="the loss's transforms: fp64 DFTs on the matrix cores, held to a derived bound (dft), or fp32 FFTs in LDS (fft: "
                         "n_fft 128, 256, 512 or 1024)")
    ap.add_argument("--epochs", type=int, default=500)
    ap.add_argument("--lr", type=float, default=5e-7)
    ap.add_argument("--no-lr-decay", action="store_true")
    ap.add_argument("--decay-from", type=int, default=80)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--optimizer", default="adam", help="adam, nadam, sgd (main_training.py:164-169) or lamb (trainer.py:37-38)")
    ap.add_argument("--weight-decay", type=float, default=0.0, help="LAMB only: tfa's weight_decay")
    ap.add_argument("--out", required=True, help="checkpoint directory (main_training.py: ../results/<name>)")
    a = ap.parse_args()
    if a.optimizer.lower() == "lamb":          # the Trainer takes LAMB as an object mirroring tfa's constructor, never as a name
        a.optimizer = U.LAMB(learning_rate=a.lr, weight_decay=a.weight_decay)
    if not torch.cuda.is_available():
        raise SystemExit("training runs on the GPU; there is none here")
    dev = torch.device("cuda:0")
    if bool(a.synthetic) == bool(a.dataset):
        raise SystemExit("give either --dataset DIR NAME or --synthetic N")
    if a.wave_loss is not None and not a.dataset:
        raise SystemExit("--wave-loss needs the target waveforms: give --dataset DIR NAME")
    if a.decay_loss is not None and not a.dataset:
        raise SystemExit("--decay-loss needs the target waveforms: give --dataset DIR NAME")
    wave = None if a.wave_loss is None else U.WaveLoss(weight=a.wave_loss, norm=a.wave_loss_norm)
    decay = None if a.decay_loss is None else U.DecayLoss(weight=a.decay_loss, floor_db=a.decay_floor_db)
    if a.spectral_loss is not None and not a.dataset:
        raise SystemExit("--spectral-loss needs the target waveforms: give --dataset DIR NAME")
    spectral = None
    if a.spectral_loss is not None:
        try:
            res = tuple(tuple(int(v) for v in r.split(":")) for r in a.spectral_resolutions.split(","))
            spectral = U.SpectralLoss(weight=a.spectral_loss, resolutions=res, floor_db=a.spectral_floor_db, method=a.spectral_method)
        except ValueError as e:
            raise SystemExit(f"--spectral-resolutions: {e}")
    wavs = wave is not None or decay is not None or spectral is not None
    if a.synthetic:
        batches = list(U.synthetic_batches(a.synthetic, a.batch, a.height, a.width, dev))
        model = build_model(a, dev)
        trainer = U.Trainer(model, lr=a.lr, alpha=a.alpha, sigmoid_loss=a.sigmoid_loss, diff_loss=a.diff_loss, beta=a.beta,
                            optimizer=a.optimizer)
        manager = U.CheckpointManager(trainer, a.out, max_to_keep=2)          # every second epoch, as with a data set
        history = U.fit(trainer, lambda epoch: batches, a.epochs, None, manager=manager, lr0=a.lr,
                        lr_exp_decay=(not a.no_lr_decay, a.decay_from))
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "history.json"), "w") as f:
            json.dump(history, f, indent=1)
        return

    dataset = U.Dataset(a.dataset[0], a.dataset[1], normalization=True, debugging=not a.no_debug, extract=a.extract,
                        room=["All"] if a.rooms == ["All"] else a.rooms, array=a.arrays, device=dev, input_shape=(a.height, a.width),
                        keep_waveforms=wavs, resample=None if a.resample == "none" else a.resample)
    # shuffle=True as main_training.py:78-79 passes it - and, as there, without effect: nothing calls on_epoch_end() (fit does
    # not either), so every epoch visits the batches in the order the seeded shuffle of the constructor gave them
    train = U.DataGenerator(dataset, batch_size=a.batch, partition="train", shuffle=True, characteristics=wavs)
    val = U.DataGenerator(dataset, batch_size=a.batch, partition="val", shuffle=True, characteristics=wavs)
    print(f"{len(dataset)} files, {len(dataset.index_in)} pairs: {len(train)} training and {len(val)} validation batches of {a.batch}")
    if len(train) == 0:
        raise SystemExit("the training partition holds less than one batch")

    model = build_model(a, dev)
    trainer = U.Trainer(model, lr=a.lr, alpha=a.alpha, sigmoid_loss=a.sigmoid_loss, diff_loss=a.diff_loss, beta=a.beta,
                        optimizer=a.optimizer, wave_loss=wave, decay_loss=decay, spectral_loss=spectral)
    manager = U.CheckpointManager(trainer, a.out, max_to_keep=2)
    start = 0
    if manager.latest_checkpoint is not None:
        epoch = manager.restore()
        start = 0 if epoch is None else epoch + 1
        print("restored", manager.latest_checkpoint, "- continuing with epoch", start + 1)
    history = U.fit(trainer, train.batches, a.epochs, val.batches if len(val) else None, manager=manager, lr0=a.lr,
                    lr_exp_decay=(not a.no_lr_decay, a.decay_from), start_epoch=start)
    with open(os.path.join(a.out, "history.json"), "w") as f:
        json.dump(history, f, indent=1)


if __name__ == "__main__":
    main()
