"""Drop-in for the reference's Ablation.py (train.py:6 ``from Ablation import *``).

Put this directory first on sys.path; ablation2 / ablation3, the layers OursLayer,
OursLayer2, OursLayer3 and GraphAttentionLayer then run on the MI355X HIP kernels with the
reference's signatures and state_dict.  ``ablation1`` is not provided yet.
"""
import torch  # noqa: F401  (the reference module exports these names)
import torch.nn as nn  # noqa: F401
import torch.nn.functional as F  # noqa: F401

import _boot  # noqa: F401
from msha_gnn_amd.layers import (GraphAttentionLayer, OursLayer, OursLayer2,  # noqa: F401
                                 OursLayer3, ablation2, ablation3)

K = 100  # Ablation.py:5 module constant
