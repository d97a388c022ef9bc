"""MI355X-native EnergyEquivGNN hot path (drop-in for the reference ``gnn`` package).

``from gnn import EnergyEquivGNN`` works as in ``scripts/train_main.py:21`` once
``energy-equiv-lattice-gnn_amd/`` is on ``sys.path``.  ``GLAMM_Dataset`` builds the
reference's graphs from catalogue entries (``gnn.lattice_data``); reading ``.lat`` files
themselves needs the un-vendored ``lattices`` package and raises.
"""
from .model import EnergyEquivGNN, GNN_Head  # noqa: F401
from .synthetic import SyntheticLattices, make_lattice  # noqa: F401
from .data import Batch, Data, DataLoader, collate, degree_stats  # noqa: F401
from .train import LightningWrappedModel, stiffness_loss  # noqa: F401
from .lattice_data import GLAMM_Dataset, RotateLat, process_lattice  # noqa: F401
from .design import (DesignLayout, DesignResult, design_layout, design_step, design_step_composed,  # noqa: F401
                     optimize_design, property_sensitivity, stiffness_sensitivity, strut_volume,
                     strut_volume_composed)
from .device_data import DeviceDataset, DeviceLoader, pack_graphs  # noqa: F401
from .metrics import (METRIC_COLUMNS, ErrorTable, aggr_errors, evaluate, metric_directions,  # noqa: F401
                      obtain_errors, stiffness_metrics, validation_metrics)
from .elastic import ELASTIC_COLUMNS, elastic_properties, elastic_properties_composed  # noqa: F401
from .transverse import (TRANSVERSE_COLUMNS, TRANSVERSE_DIR_COLUMNS, transverse_properties,  # noqa: F401
                         transverse_properties_composed)
from .optim import FlatAdamW  # noqa: F401
from .trainer import Callback, EarlyStopping, ModelCheckpoint, Trainer  # noqa: F401

__all__ = ["GLAMM_Dataset", "EnergyEquivGNN"]
classes = __all__
