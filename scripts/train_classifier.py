"""Train the room classifier deep_CNN (dl_models/cnn_clas.py) on the impulse-response tree: which of the five rooms of
`unet_rir_amd.evaluate.ROOMS` does a TARGET spectrogram come from.  One process, one GPU.

    python scripts/train_classifier.py --dataset ../datasets room_impulse --rooms All --out ../results/cnn_clas
    python scripts/train_classifier.py --synthetic 8 --epochs 3 --out ../results/cnn_clas       # no data set: 8 random batches, random labels

Data set -> `Dataset` with a device bank -> `DataGenerator(characteristics=True)` for the training and the validation partition,
whose fourth item carries the room index of every target as int32 [b] -> one-hot rows -> `deep_CNN` -> `Trainer` -> `fit` with a
`CheckpointManager`.  The one-hot rows are a torch expression on the device (`one_hot`): one small launch per step BESIDE the
train step, not part of it; a target whose room is none of the five (index -1) gets an all-zero row, which adds nothing to the
loss and counts as wrong.  `fit` reports `train_acc` / `val_acc` (correct rows over rows seen) and, as `train_amp`, the mean
cross-entropy per row.  A run continues from the latest checkpoint in --out when there is one."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import unet_rir_amd as U
from unet_rir_amd.evaluate import ROOMS


def one_hot(room, classes):
    """int32 [b] room indices -> fp32 [b, classes]; an index outside 0 .. classes - 1 gives a zero row."""
    return (room.view(-1, 1) == torch.arange(classes, device=room.device, dtype=room.dtype).view(1, -1)).to(torch.float32)


def classifier_batches(generator, classes):
    """epoch -> (target spectrogram, None, one-hot room) per batch of a DataGenerator(characteristics=True)."""
    def batches(epoch=None):
        for _, _, spec_out, (room, _) in generator.batches(epoch):
            yield spec_out, None, one_hot(room, classes)
    return batches


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dataset", nargs=2, metavar=("DIR", "NAME"), help="the tree is DIR/NAME/Room/ZoneX/...Array/*.wav")
    ap.add_argument("--synthetic", type=int, default=0, metavar="N",
                    help="instead of --dataset: N batches of synthetic_batches per epoch with random labels (a smoke run), no validation")
    ap.add_argument("--rooms", nargs="+", default=["All"], help="room names, or All")
    ap.add_argument("--arrays", nargs="+", default=["PlanarMicrophoneArray", "CircularMicrophoneArray"])
    ap.add_argument("--no-debug", action="store_true", help="load the whole tree")
    ap.add_argument("--extract", action="store_true", help="unpack the zone archives first")
    ap.add_argument("--height", type=int, default=144)
    ap.add_argument("--width", type=int, default=160)
    ap.add_argument("--no-batchnorm", action="store_true")
    ap.add_argument("--epochs", type=int, default=50)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--optimizer", default="adam", help="adam, nadam, sgd (cnn_clas.py:55-61) or lamb")
    ap.add_argument("--out", required=True, help="checkpoint directory")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("training runs on the GPU; there is none here")
    if bool(a.synthetic) == bool(a.dataset):
        raise SystemExit("give either --dataset DIR NAME or --synthetic N")
    dev, classes = torch.device("cuda:0"), len(ROOMS)
    optimizer = U.LAMB(learning_rate=a.lr) if a.optimizer.lower() == "lamb" else a.optimizer
    model = U.deep_CNN(a.height, a.width, 2, classes, not a.no_batchnorm, a.optimizer, a.lr, batch_size=a.batch, device=dev)
    model.build_model()
    model.set_optimizer_criterion()
    trainer = U.Trainer(model, lr=a.lr, optimizer=optimizer)
    manager = U.CheckpointManager(trainer, a.out, max_to_keep=2)
    start = 0
    if manager.latest_checkpoint is not None:
        epoch = manager.restore()
        start = 0 if epoch is None else epoch + 1
        print("restored", manager.latest_checkpoint, "- continuing with epoch", start + 1)

    def log(rec):
        print(f"epoch {rec['epoch']}: loss {rec['train_loss']:.4f}  train_acc {rec['train_acc']:.4f}"
              + (f"  val_acc {rec['val_acc']:.4f}" if "val_acc" in rec else ""))

    if a.synthetic:
        g = torch.Generator(device=dev)
        g.manual_seed(1)
        data = [(spec_out, None, one_hot(torch.randint(0, classes, (a.batch,), device=dev, generator=g, dtype=torch.int32), classes))
                for _, _, spec_out in U.synthetic_batches(a.synthetic, a.batch, a.height, a.width, dev)]
        train, val = (lambda epoch: data), None
    else:
        dataset = U.Dataset(a.dataset[0], a.dataset[1], normalization=True, debugging=not a.no_debug, extract=a.extract,
                            room=["All"] if a.rooms == ["All"] else a.rooms, array=a.arrays, device=dev, keep_waveforms=True,
                            input_shape=(a.height, a.width))
        tg = U.DataGenerator(dataset, batch_size=a.batch, partition="train", shuffle=True, characteristics=True)
        vg = U.DataGenerator(dataset, batch_size=a.batch, partition="val", shuffle=True, characteristics=True)
        print(f"{len(dataset)} files: {len(tg)} training and {len(vg)} validation batches of {a.batch}; classes {ROOMS}")
        if len(tg) == 0:
            raise SystemExit("the training partition holds less than one batch")
        train, val = classifier_batches(tg, classes), (classifier_batches(vg, classes) if len(vg) else None)
    history = U.fit(trainer, train, a.epochs, val, manager=manager, lr0=a.lr, lr_exp_decay=(False, 80), start_epoch=start, log=log)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "history.json"), "w") as f:
        json.dump(history, f, indent=1)
    model.save(a.out)


if __name__ == "__main__":
    main()
