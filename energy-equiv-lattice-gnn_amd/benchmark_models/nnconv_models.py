"""NNConv benchmark model (reference: scripts/benchmark_models/nnconv_models.py) -> gnn.nnconv."""
from gnn.nnconv import NNConv, NNConvNet  # noqa: F401
