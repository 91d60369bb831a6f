"""Trainer (reference trainer.py:1-164) on the HIP operator set: the same methods — set_optimizer, train, test, record, save_model —
driving PCCModel.forward_train, loss.sum_loss and the backward kernels of csrc/grad.hip.  torch.optim.Adam on the device parameters is
plumbing and stays torch.  Logging goes to `log.txt` in the log directory and to the console (no tensorboard writer).

A dataloader is any iterable of (coords [N, 4] with the batch index in column 0, feats [N, 1]) — what
`ME.utils.sparse_collate` / sparse.sparse_collate produce; pcgcv2_amd/train.py builds one from PLY files."""
import logging
import os
import time

import numpy as np
import torch

from . import loss as L
from .sparse import SparseTensor


class TrainingConfig():
    """train.py:32-43"""

    def __init__(self, logdir, ckptdir, init_ckpt, alpha, beta, lr, check_time):
        self.logdir = logdir
        os.makedirs(self.logdir, exist_ok=True)
        self.ckptdir = ckptdir
        os.makedirs(self.ckptdir, exist_ok=True)
        self.init_ckpt = init_ckpt
        self.alpha = alpha
        self.beta = beta
        self.lr = lr
        self.check_time = check_time


class Trainer():
    def __init__(self, config, model, device=None):
        self.config = config
        self.device = torch.device('cuda') if device is None else torch.device(device)
        self.logger = self.getlogger(config.logdir)
        self.model = model.to(self.device)
        self.logger.info(model)
        self.load_state_dict()
        self.epoch = 0
        self.record_set = {'bce': [], 'bces': [], 'bpp': [], 'sum_loss': [], 'metrics': []}

    def getlogger(self, logdir):
        logger = logging.getLogger(f'{__name__}.{id(self)}')
        logger.setLevel(level=logging.INFO)
        formatter = logging.Formatter('%(asctime)s: %(message)s', datefmt='%m/%d %H:%M:%S')
        handler = logging.FileHandler(os.path.join(logdir, 'log.txt'))
        handler.setLevel(logging.INFO)
        handler.setFormatter(formatter)
        console = logging.StreamHandler()
        console.setLevel(logging.INFO)
        console.setFormatter(formatter)
        logger.addHandler(handler)
        logger.addHandler(console)
        return logger

    def load_state_dict(self):
        if self.config.init_ckpt == '':
            self.logger.info('Random initialization.')
        else:
            ckpt = torch.load(self.config.init_ckpt, map_location=self.device)
            self.model.load_state_dict(ckpt['model'])
            self.logger.info('Load checkpoint from ' + self.config.init_ckpt)

    def save_model(self):
        """{'model': state_dict} in the reference's layout (PCCModel.state_dict_reference undoes what load_state_dict permutes on the way
        in), so the file loads into the reference and into coder.Coder alike -> its path"""
        path = os.path.join(self.config.ckptdir, 'epoch_' + str(self.epoch) + '.pth')
        torch.save({'model': self.model.state_dict_reference()}, path)
        return path

    def set_optimizer(self):
        params_lr_list = []
        for module_name in self.model._modules.keys():
            params_lr_list.append({'params': self.model._modules[module_name].parameters(), 'lr': self.config.lr})
        return torch.optim.Adam(params_lr_list, betas=(0.9, 0.999), weight_decay=1e-4)

    @torch.no_grad()
    def record(self, main_tag, global_step):
        self.logger.info('=' * 10 + main_tag + ' Epoch ' + str(self.epoch) + ' Step: ' + str(global_step))
        for k, v in self.record_set.items():
            self.record_set[k] = np.mean(np.array(v), axis=0)
        for k, v in self.record_set.items():
            self.logger.info(k + ': ' + str(np.round(v, 4).tolist()))
        for k in self.record_set.keys():
            self.record_set[k] = []

    def _tensor(self, coords, feats):
        return SparseTensor(features=torch.as_tensor(feats).float(), coordinates=torch.as_tensor(coords), tensor_stride=1, device=self.device)

    @torch.no_grad()
    def test(self, dataloader, main_tag='Test'):
        """trainer.py:78-104, through loss.evaluate (training=False: rounding and top-k pruning)"""
        self.logger.info('Testing Files length:' + str(len(dataloader)))
        for coords, feats in dataloader:
            rec = L.evaluate(self.model, self._tensor(coords, feats), training=False)
            self.record_set['bce'].append(rec['bce'])
            self.record_set['bces'].append(rec['bces'])
            self.record_set['bpp'].append(rec['bpp'])
            self.record_set['sum_loss'].append(rec['bce'] + rec['bpp'])
            self.record_set['metrics'].append(rec['metrics'])
        self.record(main_tag=main_tag, global_step=self.epoch)

    def step(self, x, optimizer=None, generator=None):
        """trainer.py:119-135 for one batch x: forward, sum_loss = alpha * sum_l bce_l / len(out_cls_l) + beta * bits / len(x), backward,
        optimizer step (optimizer=None: the losses only, no backward) -> {'bce', 'bces', 'bpp', 'sum_loss', 'out_set'} (floats)."""
        out_set = self.model.forward_train(x, generator=generator)
        total, bces, bpp = L.sum_loss(out_set, len(x), alpha=self.config.alpha, beta=self.config.beta)
        if optimizer is not None:
            optimizer.zero_grad()
            total.backward()
            optimizer.step()                                     # (derived.py: the step advances the stamp of every derived table — they rebuild)
        bces = [float(b) for b in bces]
        return {'bce': sum(bces), 'bces': bces, 'bpp': float(bpp), 'sum_loss': float(total), 'out_set': out_set}

    def train(self, dataloader):
        self.logger.info('=' * 40 + '\n' + 'Training Epoch: ' + str(self.epoch))
        self.optimizer = self.set_optimizer()
        self.logger.info('alpha:' + str(round(self.config.alpha, 2)) + '\tbeta:' + str(round(self.config.beta, 2)))
        self.logger.info('LR:' + str(np.round([params['lr'] for params in self.optimizer.param_groups], 6).tolist()))
        self.logger.info('Training Files length:' + str(len(dataloader)))
        start_time = time.time()
        batch_step = 0
        for batch_step, (coords, feats) in enumerate(dataloader):
            rec = self.step(self._tensor(coords, feats), self.optimizer)
            with torch.no_grad():
                out_set = rec['out_set']
                metrics = [L.get_metrics(out_cls, ground_truth)
                           for out_cls, ground_truth in zip(out_set['out_cls_list'], out_set['ground_truth_list'])]
                self.record_set['bce'].append(rec['bce'])
                self.record_set['bces'].append(rec['bces'])
                self.record_set['bpp'].append(rec['bpp'])
                self.record_set['sum_loss'].append(rec['bce'] + rec['bpp'])
                self.record_set['metrics'].append(metrics)
                if (time.time() - start_time) > self.config.check_time * 60:
                    self.record(main_tag='Train', global_step=self.epoch * len(dataloader) + batch_step)
                    self.save_model()
                    start_time = time.time()
        with torch.no_grad():
            self.record(main_tag='Train', global_step=self.epoch * len(dataloader) + batch_step)
        self.save_model()
        self.epoch += 1
