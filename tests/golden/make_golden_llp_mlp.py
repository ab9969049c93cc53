"""Writes tests/golden/llp_mlp.npz: the reference's 'mlp' ``LinkPredictor`` (LLP.py:86-115)
under the training objective of LLP.py:233, :235 and :238, in float64 and eval mode.

    python tests/golden/make_golden_llp_mlp.py /path/to/the/reference/checkout

LLP.py runs as a script, so ``LinkPredictor`` is taken out of its syntax tree and executed on
its own, as make_golden_llp_student.py does.  Needs the reference checkout; the tests only
read the .npz (numeric arrays only).

n = 40 table rows, F = N = 32, P = 96 pairs, none of them padding (dst < 32 so that it is a
class label, as LLP.py:235 uses it).  Stored: ``h``, ``src``, ``dst``, ``W``, ``b`` (the first
Linear of ``LinkPredictor('mlp', 32, 32, 1, 2, 0.5)`` after ``torch.manual_seed(3)``),
``t_out``, ``true_label``, ``kd_p``; ``output`` (P, N), ``label_loss``, ``mse``, ``loss`` =
true_label * label_loss + kd_p * mse, and the autograd gradients ``dh``, ``dW``, ``db``.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

from make_golden_llp_student import extract

N_ROWS, FEAT, PAIRS = 40, 32, 96
TRUE_LABEL, KD_P = 10.0, 100.0


def main(reference):
    LinkPredictor = extract(os.path.join(reference, "LLP.py"), {"LinkPredictor"})["LinkPredictor"]
    torch.manual_seed(3)
    predictor = LinkPredictor("mlp", FEAT, FEAT, 1, 2, 0.5).double()
    predictor.eval()
    g = torch.Generator().manual_seed(11)
    h = (torch.randn(N_ROWS, FEAT, generator=g, dtype=torch.float64) * 0.8).requires_grad_(True)
    source_index = torch.randint(0, N_ROWS, (PAIRS,), generator=g)
    recipient_index = torch.randint(0, FEAT, (PAIRS,), generator=g)
    t_out = torch.rand(PAIRS, FEAT, generator=g, dtype=torch.float64)
    output = predictor(h[source_index], h[recipient_index]).squeeze()      # LLP.py:233
    label_loss = F.nll_loss(output, recipient_index)                       # LLP.py:235
    mse = F.mse_loss(output, t_out)                                        # LLP.py:238
    loss = TRUE_LABEL * label_loss + KD_P * mse
    loss.backward()
    lin = predictor.lins[0]
    assert predictor.lins[1].weight.grad is None
    z = dict(h=h.detach().numpy(), src=source_index.numpy(), dst=recipient_index.numpy(),
             W=lin.weight.detach().numpy(), b=lin.bias.detach().numpy(), t_out=t_out.numpy(),
             true_label=np.float64(TRUE_LABEL), kd_p=np.float64(KD_P),
             output=output.detach().numpy(), label_loss=label_loss.detach().numpy(),
             mse=mse.detach().numpy(), loss=loss.detach().numpy(), dh=h.grad.numpy(),
             dW=lin.weight.grad.numpy(), db=lin.bias.grad.numpy())
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "llp_mlp.npz")
    np.savez_compressed(path, **{k: np.ascontiguousarray(v) for k, v in z.items()})
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
