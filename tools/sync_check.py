#!/usr/bin/env python3
"""Report host<->device synchronisations inside the training step, fed a resident batch and a
fresh batch per step (torch.cuda.set_sync_debug_mode('warn') around a step after warm-up)."""
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "energy-equiv-lattice-gnn_amd")]

import torch  # noqa: E402


def main():
    import bench
    from gnn import EnergyEquivGNN
    from gnn.data import collate
    from gnn.synthetic import SyntheticLattices
    from gnn.train import stiffness_loss
    ds = SyntheticLattices(4, 1024, 4096, 1234)
    batch = collate([ds[g] for g in range(4)]).to("cuda")
    torch.manual_seed(0)
    model = EnergyEquivGNN(bench.make_params(4, ds.max_edge_radius)).cuda()
    model.edge_graph(batch)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3, amsgrad=True, fused=True)
    plist = list(model.parameters())

    # three feeds: the resident batch (bench.py's form), a fresh DeviceLoader batch per step and a
    # freshly collated batch moved to the device per step (fresh batches bring no strut map)
    from gnn import DeviceDataset, DeviceLoader
    loader = DeviceLoader(DeviceDataset(ds, "cuda"), 4)
    feeds = {"resident batch": lambda: batch,
             "fresh DeviceLoader batch": lambda: loader.assemble([0, 1, 2, 3]),
             "fresh collated batch": lambda: collate([ds[g] for g in range(4)]).to("cuda")}

    def step(b):
        opt.zero_grad(set_to_none=True)
        loss = stiffness_loss(model(b)["stiffness"], b.stiffness)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(plist, 10.0)
        opt.step()
    for name, feed in feeds.items():
        for _ in range(2):
            step(feed())
        b = feed()
        torch.cuda.synchronize()
        with warnings.catch_warnings(record=True) as ws:
            warnings.simplefilter("always")
            torch.cuda.set_sync_debug_mode("warn")
            step(b)
            torch.cuda.set_sync_debug_mode(0)
        torch.cuda.synchronize()
        strut = getattr(model.edge_graph(b, build=False), "strut", None)
        print(f"{name}: {len(ws)} synchronising calls in one step (strut map: "
              f"{'none' if strut is None else str(strut.n_rows) + ' rows'})")
        for w in ws[:20]:
            print(" -", str(w.message)[:160], f"({w.filename}:{w.lineno})")


if __name__ == "__main__":
    main()
