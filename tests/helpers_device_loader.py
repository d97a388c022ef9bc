"""The five-graph fixture dataset of the device-loader tests: three catalogue-style entries
(17 / 24 / 31 nodes, two relative densities each, through ``GLAMM_Dataset`` + ``scale_targets``
as ``tests/test_gpu_datapath.py`` builds them) of which graphs 0..2 are kept, a single node
without edges, and a graph with isolated nodes (repeated ``rowptr`` entries in the middle and at
the end).  Items are untransformed: cartesian fp32 targets, what ``RotateLat`` takes."""
from __future__ import annotations

import numpy as np
import torch

SEL = [3, 0, 4, 1, 3]     # repeats an id, starts and ends on different sizes


def _targets(seed: int):
    from gnn.lattice_data import mandel_to_cart4
    rng = np.random.default_rng(seed)
    a = rng.normal(size=(6, 6))
    stiff = a @ a.T / 6 + 0.5 * np.eye(6)
    comp = np.linalg.inv(stiff)
    return (torch.from_numpy(mandel_to_cart4(stiff)).unsqueeze(0).float(),
            torch.from_numpy(mandel_to_cart4(comp)).unsqueeze(0).float())


def single_node():
    from gnn.data import Data
    c, s = _targets(40)
    return Data(name="single", positions=torch.tensor([[0.1, 0.2, 0.3]]), node_attrs=torch.ones(1, 1),
                edge_index=torch.zeros(2, 0, dtype=torch.long), shifts=torch.zeros(0, 3),
                edge_attr=torch.zeros(0, 1), rel_dens=0.02, stiffness=c, compliance=s)


def isolated_nodes():
    """7 nodes; nodes 2 and 6 carry no edge (node 6 is the last), node 4 only sends."""
    from gnn.data import Data
    rng = np.random.default_rng(41)
    und = [(0, 1), (1, 3), (3, 5), (5, 0), (0, 3)]
    snd = [a for a, b in und] + [b for a, b in und] + [4, 4]
    rcv = [b for a, b in und] + [a for a, b in und] + [0, 5]
    e = len(snd)
    c, s = _targets(42)
    return Data(name="isolated", positions=torch.tensor(rng.random((7, 3)) * 0.6, dtype=torch.float32),
                node_attrs=torch.ones(7, 1), edge_index=torch.tensor([snd, rcv], dtype=torch.long),
                shifts=torch.tensor(rng.integers(-1, 2, size=(e, 3)) * 0.7, dtype=torch.float32),
                edge_attr=torch.tensor(rng.uniform(0.005, 0.05, size=(e, 1)), dtype=torch.float32),
                rel_dens=0.05, stiffness=c, compliance=s)


def five_graphs():
    """[17 nodes @ 0.01, 24 nodes @ 0.03, 31 nodes @ 0.01, single node, isolated nodes] as ``Data``."""
    from gnn.lattice_data import GLAMM_Dataset
    from test_gpu_datapath import random_entry
    ents = [random_entry("c", 17, 3), random_entry("a", 24, 1), random_entry("b", 31, 2)]
    ds = GLAMM_Dataset(ents, n_reldens=2)
    ds.scale_targets(reldens_norm=True)
    it = ds.items      # c@0.01, c@0.03, a@0.01, a@0.03, b@0.01, b@0.03
    return [it[0], it[3], it[4], single_node(), isolated_nodes()]


def collated(items, sel, Q=None):
    """``collate`` of ``RotateLat`` applied to the selected items (``Q``: [B, 3, 3] or None)."""
    from gnn.data import collate
    from gnn.lattice_data import RotateLat
    if Q is None:
        return collate([RotateLat(rotate=False)(items[i]) for i in sel])
    return collate([RotateLat()(items[i], Q=Q[k]) for k, i in enumerate(sel)])
