"""unet-rir_amd: MI355X (gfx950) implementation of the igmsalinas/unet-rir U-Net train-step hot path.

Host side in Python over a C ABI (include/unetrir.h) of hand-written HIP kernels; PyTorch provides
device memory, streams and torch.distributed only.
"""
from . import _lib, build, callbacks, evaluate, ops  # noqa: F401
from ._lib import UnetrirError  # noqa: F401
from .engine import UNetEngine  # noqa: F401
from .device import HipRuntime  # noqa: F401
from .ae import AutoencoderEngine  # noqa: F401
from .aenet import AENetEngine  # noqa: F401
from .cnn_clas import DeepCNNEngine, deep_CNN  # noqa: F401
from .diffunet import DiffUNetEngine  # noqa: F401
from .diffvae import DiffVAEEngine  # noqa: F401
from .model import VAE, VQVAE, AENet, Autoencoder, DiffUNet, DiffVAE, ResAE, UNet  # noqa: F401
from .resae import ResAEEngine  # noqa: F401
from .unet_graph import UNetGraphEngine  # noqa: F401
from .vae import VAEEngine  # noqa: F401
from .vqvae import VQVAEEngine  # noqa: F401
from .data import DeviceBatchPipeline, synthetic_batches  # noqa: F401
from .evaluate import Evaluator, acoustics, score, write_report  # noqa: F401
from .dataset import DataGenerator, Dataset, read_wav  # noqa: F401
from .lamb import LAMB  # noqa: F401
from .trainer import CheckpointManager, GradBucketer, Trainer, fit, lr_schedule  # noqa: F401
from .waveloss import WaveLoss  # noqa: F401
from .decayloss import DecayLoss  # noqa: F401
from .spectralloss import SpectralLoss  # noqa: F401
from .auralize import AuralizeStream, auralize, auralize_path  # noqa: F401
from .resample import Resampler, resample  # noqa: F401

__all__ = ["ops", "build", "UnetrirError", "UNetEngine", "UNetGraphEngine", "ResAEEngine", "UNet", "ResAE", "Autoencoder", "AutoencoderEngine", "VAE", "VAEEngine", "VQVAE", "VQVAEEngine", "AENet", "AENetEngine", "DiffUNet", "DiffUNetEngine", "DiffVAE", "DiffVAEEngine", "deep_CNN", "DeepCNNEngine", "HipRuntime", "Trainer", "WaveLoss", "DecayLoss", "SpectralLoss", "LAMB", "GradBucketer", "lr_schedule", "CheckpointManager", "fit", "DeviceBatchPipeline", "synthetic_batches", "evaluate", "Evaluator", "score", "acoustics", "write_report", "Dataset", "DataGenerator", "read_wav", "auralize", "auralize_path", "AuralizeStream", "Resampler", "resample"]
