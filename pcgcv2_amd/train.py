"""Training CLI (reference train.py) with the reference's flags and defaults.  The dataset is a glob of cloud files.  Without a loader
flag the files are ASCII PLY, re-read for every batch by PlyLoader and collated by sparse_collate on the host.  With --num_workers,
--device_cache or --augment the loaders come from data_loader.make_data_loader: clouds are cached after the first read,
on the GPU under --device_cache, and the reference's HDF5 patch files (.h5) are read too where h5py is installed.

    python -m pcgcv2_amd.train --dataset 'clouds/*.ply' --batch_size 8 --epoch 50 --prefix tp
    python -m pcgcv2_amd.train --dataset 'clouds/*.ply' --batch_size 8 --epoch 50 --prefix tp --device_cache --augment --num_workers 4
"""
import argparse
import glob
import os
import random

import torch

from .data_utils import read_ply_ascii_geo
from .pcc_model import PCCModel
from .sparse import sparse_collate
from .trainer import Trainer, TrainingConfig


def parse_args(argv=None):
    parser = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument('--dataset', default='./training_dataset/*.ply', help='glob of ASCII PLY files')
    parser.add_argument('--dataset_num', type=int, default=int(2e4))
    parser.add_argument('--alpha', type=float, default=1., help='weights for distoration.')
    parser.add_argument('--beta', type=float, default=1., help='weights for bit rate.')
    parser.add_argument('--init_ckpt', default='')
    parser.add_argument('--lr', type=float, default=8e-4)
    parser.add_argument('--batch_size', type=int, default=8)
    parser.add_argument('--epoch', type=int, default=50)
    parser.add_argument('--check_time', type=float, default=10, help='frequency for recording state (min).')
    parser.add_argument('--prefix', type=str, default='tp', help='prefix of checkpoints/logger, etc.')
    parser.add_argument('--num_workers', type=int, default=0, help='host threads parsing files ahead of the training loop (data_loader).')
    parser.add_argument('--device_cache', action='store_true', help='keep every cloud read so far on the GPU and collate batches there.')
    parser.add_argument('--augment', action='store_true', help='one of the 48 symmetries of the cube per training cloud and batch.')
    return parser.parse_args(argv)


class PlyLoader:
    """batches of (coords [N, 4], feats [N, 1]) from PLY files: any iterable of such pairs is a dataloader to Trainer"""

    def __init__(self, files, batch_size, shuffle):
        self.files, self.batch_size, self.shuffle = list(files), int(batch_size), shuffle

    def __len__(self):
        return (len(self.files) + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        files = list(self.files)
        if self.shuffle:
            random.shuffle(files)
        for i in range(0, len(files), self.batch_size):
            clouds = [torch.tensor(read_ply_ascii_geo(f)).int() for f in files[i:i + self.batch_size]]
            yield sparse_collate(clouds, [torch.ones((len(c), 1)) for c in clouds])


def main(argv=None):
    args = parse_args(argv)
    config = TrainingConfig(logdir=os.path.join('./logs', args.prefix), ckptdir=os.path.join('./ckpts', args.prefix), init_ckpt=args.init_ckpt,
                            alpha=args.alpha, beta=args.beta, lr=args.lr, check_time=args.check_time)
    trainer = Trainer(config=config, model=PCCModel())
    filedirs = sorted(glob.glob(args.dataset))[:int(args.dataset_num)]
    if not filedirs:
        raise SystemExit(f'no file matches {args.dataset!r}')
    n_test = round(len(filedirs) / 10)
    if args.num_workers or args.device_cache or args.augment:
        from .data_loader import PCDataset, make_data_loader
        train_loader = make_data_loader(PCDataset(filedirs[n_test:]), args.batch_size, shuffle=True, num_workers=args.num_workers,
                                        device_cache=args.device_cache, augment=args.augment, device=trainer.device if args.device_cache else None)
        test_loader = make_data_loader(PCDataset(filedirs[:n_test]), args.batch_size, shuffle=False, num_workers=args.num_workers,
                                       device_cache=args.device_cache, augment=False, device=trainer.device if args.device_cache else None)
    else:
        train_loader = PlyLoader(filedirs[n_test:], args.batch_size, shuffle=True)
        test_loader = PlyLoader(filedirs[:n_test], args.batch_size, shuffle=False)
    for epoch in range(0, args.epoch):
        if epoch > 0:
            trainer.config.lr = max(trainer.config.lr / 2, 1e-5)
        trainer.train(train_loader)
        if len(test_loader):
            trainer.test(test_loader, 'Test')


if __name__ == '__main__':
    main()
