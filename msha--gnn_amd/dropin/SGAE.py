"""Drop-in classes of the reference's SGAE.py (the script itself is a training driver whose
dataset class does not exist): the GraphSAGE baseline with forward(source_index, adj), and
the names the script takes from ``from model import *``."""
import numpy as np  # noqa: F401
import torch  # noqa: F401
import torch.nn as nn  # noqa: F401
import torch.nn.functional as F  # noqa: F401

import _boot  # noqa: F401
from msha_gnn_amd.graph import normalize_adjacency_matrix  # noqa: F401
from msha_gnn_amd.layers import GraphSAGE  # noqa: F401
from msha_gnn_amd.metrics import (Evaluator, calculate_accuracy, calculate_auc,  # noqa: F401
                                  calculate_precision_recall)
