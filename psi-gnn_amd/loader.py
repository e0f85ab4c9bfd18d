"""Stand-ins for the three torch_geometric pieces the reference's scripts wrap around the model
(``dirichlet/psignn/main.py:9-10,70-78,106``; ``test/test_func.py:134-140``): ``DataListLoader``, ``DataLoader`` and
``DataParallel``.  No torch_geometric is needed.

* ``DataListLoader(dataset, batch_size, shuffle)`` yields python lists of graphs (as PyG's does);
* ``DataLoader(dataset, batch_size, shuffle)`` yields disjoint-union batches (``data.collate``);
* ``DataParallel(module)`` keeps the reference's calling convention -- ``model(list_of_graphs)``, ``model.module`` -- but
  is one process per GPU by design: the list is collated into ONE union batch on the module's device (what PyG's
  DataParallel does on each of its devices) and handed to the module.  Multi-GPU data parallelism is done with one process
  per GPU and ``training_class.allreduce_mean_grads`` (RCCL), not with replica threads.  ``DataParallel(module, replicas=R)``
  gives the reference's R independent replicas on ONE GPU: R union batches, solved in lockstep (see the class).
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .data.meshdata import collate


class DataListLoader:
    def __init__(self, dataset, batch_size=1, shuffle=False, generator=None, **_ignored):
        self.dataset, self.batch_size, self.shuffle, self.generator = dataset, int(batch_size), bool(shuffle), generator

    def __len__(self):
        return (len(self.dataset) + self.batch_size - 1) // self.batch_size

    def _order(self):
        n = len(self.dataset)
        return torch.randperm(n, generator=self.generator).tolist() if self.shuffle else list(range(n))

    def __iter__(self):
        order = self._order()
        for i in range(0, len(order), self.batch_size):
            yield [self.dataset[j] for j in order[i:i + self.batch_size]]


class DataLoader(DataListLoader):
    def __iter__(self):
        for graphs in super().__iter__():
            yield collate(graphs)


class DataParallel(nn.Module):
    """``replicas = 1`` (default): the list is collated into one union batch.  ``replicas = R > 1``: the reference's
    ``num_gpus = R`` semantics on one GPU (``dirichlet/psignn/main.py:106``) -- the list is cut into ``min(R, len(list))``
    contiguous chunks of near-equal graph count (the first ``len % R`` chunks hold one graph more), each collated to a union
    batch of its own, and the module is handed the list of them: R independent fixed-point problems solved in lockstep
    (``ModelDEQDSS.forward`` on a list), every value of the returned ``loss_dic`` of shape ``(R,)``."""

    def __init__(self, module, device_ids=None, output_device=None, replicas=1):
        super().__init__()
        if int(replicas) < 1:
            raise ValueError(f"replicas must be >= 1, got {replicas!r}")
        self.module = module
        self.replicas = int(replicas)

    def _device(self):
        return next(self.module.parameters()).device

    def forward(self, data_list):
        if isinstance(data_list, (list, tuple)):
            if len(data_list) == 0:
                raise ValueError("DataParallel received an empty list of graphs")
            if self.replicas > 1:
                graphs, dev = list(data_list), self._device()
                r = min(self.replicas, len(graphs))
                base, extra = divmod(len(graphs), r)
                chunks, at = [], 0
                for i in range(r):
                    n = base + (1 if i < extra else 0)
                    chunks.append(graphs[at] if n == 1 else collate(graphs[at:at + n]))
                    at += n
                return self.module([c.to(dev) for c in chunks])
            batch = data_list[0] if len(data_list) == 1 else collate(list(data_list))
        else:
            batch = data_list
        return self.module(batch.to(self._device()))
