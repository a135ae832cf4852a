"""Score a trained model on a test set, on the device, and write the reference's three report files
(rir_generation.py:160-532 -> unet_rir_amd.Evaluator + write_report).

    python scripts/evaluate.py --load SAVED_MODEL_DIR --data BATCH_DIR --out REPORT_DIR [--name unet] [--diff-gen]
    python scripts/evaluate.py --checkpoint CKPT_DIR --filters 32 --kernels 3 --data BATCH_DIR --out REPORT_DIR
    python scripts/evaluate.py --checkpoint CKPT_DIR --dataset DIR NAME [--rooms ...] [--arrays ...] --out REPORT_DIR
    python scripts/evaluate.py --synthetic 8 --out REPORT_DIR            # no dataset, no checkpoint: random weights and data

--load         a folder written by `UNet.save` / `ResAE.save` / `Autoencoder.save` / `VAE.save` / `VQVAE.save` (--arch picks the class)
--checkpoint   a `CheckpointManager` directory; the latest checkpoint is restored into a U-Net built from --filters / --kernels
               (--arch vae: into the VAE of rir_generation.py:78-87, latent size --latent; --arch vqvae: into the VQ-VAE of
               dl_models/vqvae.py:522-531; --arch aenet / diffunet: from --filters; --arch diffvae: the model of diff_vae.py:476-485)
--data         a directory of .npz files, one test batch each: spec_in, spec_out fp32 [B, H, W, 2] (or [B, 2, H, W]), emb int
               [B, 2, 16], wav_true fp32 [B, T], room = B room names (or indices into evaluate.ROOMS)
--dataset      the impulse-response tree DIR/NAME/Room/ZoneX/...Array/*.wav itself: the test partition of `unet_rir_amd.Dataset`
               with characteristics=True, shuffle=False, as rir_generation.py:67-70 (--rooms / --arrays filter it, default all)
--synthetic N  N batches of `synthetic_batches`, which yields no waveforms: wav_true is the reconstruction of spec_out
--algorithm    ph (default): reconstruct from the predicted phase; gl: Griffin-Lim from the predicted magnitude
               (rir_generation.py:62, :137; --gl-iters, --gl-momentum, --gl-seed; --gl-method fft: the fp32 FFT form of the loop)
--acoustics    also score the room-acoustic figures (arrival of the direct sound, direct-to-reverberant ratio, C50, centre time,
               early decay time) of predicted against true waveform and write a fourth file, NAME_acoustics.csv
"""
import argparse
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import unet_rir_amd as U
from unet_rir_amd.features import PostProcess


def build_model(a, dev):
    cls = {"unet": U.UNet, "resae": U.ResAE, "ae": U.Autoencoder, "vae": U.VAE, "vqvae": U.VQVAE, "aenet": U.AENet,
           "diffunet": U.DiffUNet, "diffvae": U.DiffVAE}[a.arch]
    if a.load:
        return cls.load(a.load, batch_size=a.batch, device=dev)
    if a.arch in ("vae", "vqvae", "diffvae"):
        if a.arch == "diffvae":    # the model of dl_models/diff_vae.py's own __main__ block (:476-485); score it with --diff-gen
            m = U.DiffVAE((a.height, a.width, 2), (2, 16), conv_filters=(32, 64, 128, 256), conv_kernels=(3, 3, 3, 3),
                          conv_strides=(2, 2, 2, 2), latent_space_dim=16, n_neurons=20 * 64, batch_size=a.batch, device=dev, dropout=False)
        elif a.arch == "vae":    # as rir_generation.py:78-87 builds it (latent 32 there, 64 in main_training.py:143-152: --latent)
            m = U.VAE((a.height, a.width, 2), (2, 16), conv_filters=(64, 128, 256, 512), conv_kernels=(3, 3, 3, 3),
                      conv_strides=(2, 2, 2, 2), latent_space_dim=a.latent, n_neurons=32 * 64, name=a.name, batch_size=a.batch, device=dev,
                      dropout=False)
        else:                  # the model of dl_models/vqvae.py's own __main__ block (:522-531)
            m = U.VQVAE((a.height, a.width, 2), (2, 16), conv_filters=(32, 64, 128, 256), conv_kernels=(3, 3, 3, 3),
                        conv_strides=(2, 2, 2, 2), latent_space_dim=16, n_neurons=320, name=a.name, batch_size=a.batch, device=dev,
                        dropout=False)
        if a.checkpoint:
            mgr = U.CheckpointManager(U.Trainer(m.engine, dropout=False), a.checkpoint)
            if mgr.latest_checkpoint is None:
                raise SystemExit(f"no checkpoint in {a.checkpoint}")
            mgr.restore()
            print("restored", mgr.latest_checkpoint)
        return m
    if a.arch not in ("unet", "aenet", "diffunet"):
        raise SystemExit("--checkpoint and --synthetic without --load build a U-Net, an AENet, a DiffUNet, a VAE, a DiffVAE or a VQ-VAE; "
                         "use --load for the other autoencoders")
    if a.arch == "diffunet":       # score it with --diff-gen (rir_generation.py:51-63)
        m = U.DiffUNet((a.height, a.width, 2), (2, 16), number_filters_0=a.filters, batch_size=a.batch, device=dev, dropout=False)
    elif a.arch == "aenet":
        m = U.AENet((a.height, a.width, 2), (2, 16), number_filters_0=a.filters, batch_size=a.batch, device=dev, dropout=False)
    else:
        m = U.UNet((a.height, a.width, 2), (2, 16), number_filters_0=a.filters, kernels=a.kernels, batch_size=a.batch, device=dev,
                   dropout=False)
    if a.checkpoint:
        mgr = U.CheckpointManager(U.Trainer(m.engine, dropout=False), a.checkpoint)
        if mgr.latest_checkpoint is None:
            raise SystemExit(f"no checkpoint in {a.checkpoint}")
        mgr.restore()
        print("restored", mgr.latest_checkpoint)
    return m


def file_batches(folder, dev):
    files = sorted(glob.glob(os.path.join(folder, "*.npz")))
    if not files:
        raise SystemExit(f"no .npz batches in {folder}")
    for f in files:
        with np.load(f) as z:
            room = z["room"]
            room = [str(r) for r in room] if room.dtype.kind in "US" else torch.from_numpy(room.astype(np.int32)).to(dev)
            yield (torch.from_numpy(z["spec_in"]).float().to(dev), torch.from_numpy(z["emb"]).to(dev),
                   torch.from_numpy(z["spec_out"]).float().to(dev), torch.from_numpy(z["wav_true"]).float().to(dev), room)


def dataset_batches(a, dev):
    ds = U.Dataset(a.dataset[0], a.dataset[1], normalization=True, room_characteristics=True, room=a.rooms, array=a.arrays,
                   device=dev, keep_waveforms=True, input_shape=(a.height, a.width),
                   resample=None if a.resample == "none" else a.resample)
    gen = U.DataGenerator(ds, batch_size=a.batch, partition="test", shuffle=False, characteristics=True)
    if len(gen) == 0:
        raise SystemExit(f"the test partition ({len(gen.index_in)} pairs) holds less than one batch of {a.batch}")
    for spec_in, emb, spec_out, (room, wav_true) in gen:
        yield spec_in, emb, spec_out, wav_true, room


def synthetic(a, dev):
    post = PostProcess()
    for k, (spec_in, emb, spec_out) in enumerate(U.synthetic_batches(a.synthetic, a.batch, a.height, a.width, dev)):
        room = [U.evaluate.ROOMS[(k * a.batch + j) % len(U.evaluate.ROOMS)] for j in range(a.batch)]
        yield spec_in, emb, spec_out, post.post_process(spec_out).clone(), room


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--load")
    ap.add_argument("--checkpoint")
    ap.add_argument("--arch", choices=("unet", "resae", "ae", "vae", "vqvae", "aenet", "diffunet", "diffvae"), default="unet")
    ap.add_argument("--latent", type=int, default=32, help="latent_space_dim of --arch vae built without --load")
    ap.add_argument("--filters", type=int, default=32)
    ap.add_argument("--kernels", type=int, default=3)
    ap.add_argument("--height", type=int, default=144)
    ap.add_argument("--width", type=int, default=160)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--data")
    ap.add_argument("--dataset", nargs=2, metavar=("DIR", "NAME"))
    ap.add_argument("--rooms", nargs="+", default=None, help="with --dataset: room names (default: all five)")
    ap.add_argument("--arrays", nargs="+", default=None, help="with --dataset: array names (default: both)")
    ap.add_argument("--resample", choices=("none", "kaiser_best", "kaiser_fast"), default="none",
                    help="with --dataset: files of --dataset that are not at the data set's rate: none (an error), or converted on the device (librosa's res_type names)")
    ap.add_argument("--synthetic", type=int, default=0)
    ap.add_argument("--diff-gen", action="store_true")
    ap.add_argument("--algorithm", choices=("ph", "gl"), default="ph")
    ap.add_argument("--gl-iters", type=int, default=32)
    ap.add_argument("--gl-momentum", type=float, default=0.99)
    ap.add_argument("--gl-seed", type=int, default=0)
    ap.add_argument("--gl-method", choices=("dft", "fft"), default="dft",
                    help="dft: fp64, held to a bound per element; fft: fp32 FFTs in LDS, librosa's own precision, faster")
    ap.add_argument("--acoustics", action="store_true")
    ap.add_argument("--out", required=True)
    ap.add_argument("--name", default="unet")
    a = ap.parse_args()
    if bool(a.data) + bool(a.synthetic) + bool(a.dataset) != 1:
        raise SystemExit("give exactly one of --data, --dataset and --synthetic")
    if not torch.cuda.is_available():
        raise SystemExit("evaluation runs on the GPU; there is none here")
    dev = torch.device("cuda:0")
    model = build_model(a, dev)
    ev = U.Evaluator(model, diff_gen=a.diff_gen, algorithm=a.algorithm, gl_iters=a.gl_iters, gl_momentum=a.gl_momentum,
                     gl_seed=a.gl_seed, gl_method=a.gl_method, acoustics=a.acoustics)
    for batch in (file_batches(a.data, dev) if a.data else dataset_batches(a, dev) if a.dataset else synthetic(a, dev)):
        ev.update(*batch)
    res = ev.result()
    for p in U.write_report(res, a.out, a.name):
        print("wrote", p)
    print("samples", res["n"][0], " ".join(f"{m}={res[m][0]:.6g}" for m in U.evaluate.METRICS))
    if a.acoustics:
        print("acoustics", " ".join(f"{m}={v['err'][0]:.6g} (n={v['n'][0]})" for m, v in res["acoustics"].items()))


if __name__ == "__main__":
    main()
