"""Drop-in classes of the reference's LLP.py (the script itself is a training
driver): LinkPredictor, the student MLP, KD_cosine and the teacher GAT with
forward(input, adj)."""
import torch  # noqa: F401
import torch.nn as nn  # noqa: F401
import torch.nn.functional as F  # noqa: F401

import _boot  # noqa: F401
from msha_gnn_amd.functional import link_match_loss
from msha_gnn_amd.layers import MLP, GraphAttentionLayer, LinkPredictor  # noqa: F401
from msha_gnn_amd.layers import LLPGAT as GAT  # noqa: F401

Teacher_LinkPredictor = LinkPredictor  # LLP.py:170-198 is the same module


def KD_cosine(s, t):  # noqa: N802  (reference function name)
    """LLP.py:34-35: ``1 - cosine_similarity(s, t.detach(), dim=-1).mean()`` on rows already
    gathered, (B, F) each."""
    return link_match_loss(s, None, t)
