"""``Adam``: train.py's optimizer (train.py:207 ``optim.Adam(model.parameters(), lr,
weight_decay)``, stepped at :232) as one HIP launch over every parameter
(``msha_adam_step``, csrc/optim.hip).

Same update as ``torch.optim.Adam`` (L2 weight decay; no amsgrad / maximize), same
constructor and ``state_dict`` layout (``step``, ``exp_avg``, ``exp_avg_sq`` per
parameter; the moments in the parameter's dtype).  The step counts live on the device,
so a captured HIP graph (step.GraphedStep) replays the update with the right bias
corrections.

``fuse_dropout_grad(param)``: the parameter's only consumer is the models' feature
dropout (``Sfeatures``, Ablation.py:296 / Ours.py:161).  Its backward then hands the
dropout's OUTPUT gradient and mask seed to this optimizer instead of materialising the
parameter's gradient, and ``step()`` folds the mask into its gradient read: the 5M-float
gradient is never written or re-read, and every parameter still updates in ONE launch
at ``step()``.  The parameter's ``.grad`` stays None.  (One backward per step for a fused
parameter: a second backward before ``step()`` raises, as accumulation would need the
gradient this path never forms.)

``fuse_row_grad(param)``: an embedding-style table trained by ``functional.link_bce_loss``,
``link_distill_loss``, ``link_mlp_loss``, ``link_match_loss`` or ``sage_forward``.  Their
backward hands this optimizer the gradient of the rows the batch touches
(``functional.RowGrad``) instead of an (n, F) ``.grad``, and ``step()`` runs
``msha_adam_rows_step`` over those rows: the same update with one global step count, the
other rows neither read nor written.  With ``accumulate=True`` up to four such gradients of
one table (LLP's label + matching + distillation terms) are summed before the step
(``msha_row_grad_union``).  ``state_dict`` is unchanged.

``fuse_row_grad(param, replay=True)``: the same row path with the *dense* optimizer's
trajectory, weight decay included (``msha_adam_rows_replay``).  The state gains ``row_step``,
one int32 per row: the step after which the row in memory is valid.  A row that no batch
names falls behind; the steps it missed (zero gradient plus ``weight_decay * p``) are replayed
in registers when the row is next read or stepped, with each step's own bias corrections, so
after ``catch_up(param)`` the table and both moments hold the bits of the unregistered run.
The five losses above catch up the rows they read; every other reader of the table
(``score_pairs``, ``topk_inner``, ``rank_inner``, indexing, a view, a cast, a checkpoint for
another optimizer) calls ``opt.catch_up(table)`` first.
"""
from __future__ import annotations

import ctypes
import weakref

import torch

from . import _lib

_DT = {torch.float32: 0, torch.bfloat16: 1}
MAX_ROW_GRADS = _lib.MAX_ROW_LISTS  # pending row gradients of a fuse_row_grad(accumulate=True) table
# Replayed steps per row in one launch of catch_up(param)'s flush over the whole table: a
# launch is bounded by n * F * FLUSH_CHUNK element updates (2M x 128 rows: 2.7e11, a fraction
# of a second), and a flush after T steps takes ceil(T / FLUSH_CHUNK) launches.  Four of the
# kernel's 256-step scalar windows.
FLUSH_CHUNK = 1024
_ALL_STEPS = 2 ** 31 - 1  # max_steps of a launch that must bring its rows to the present


class Adam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0,
                 amsgrad=False, *, maximize=False, foreach=None, capturable=True,
                 differentiable=False, fused=None):
        if amsgrad or maximize or differentiable:
            raise NotImplementedError("msha Adam: amsgrad / maximize / differentiable")
        if not 0.0 <= lr or not 0.0 <= eps or not 0.0 <= weight_decay:
            raise ValueError("msha Adam: lr, eps and weight_decay must be >= 0")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError("msha Adam: betas must be in [0, 1)")
        # capturable / fused in the defaults: torch's load_state_dict then moves every
        # loaded 'step' to the parameter's device as fp32 (a CPU step from a
        # map_location='cpu' checkpoint or a torch.optim.Adam state_dict would otherwise
        # stay on the host, and the kernel reads it through a device pointer)
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps,
                                      weight_decay=weight_decay, amsgrad=False,
                                      maximize=False, foreach=None, capturable=True,
                                      differentiable=False, fused=False))
        self._ws = {}  # device -> the launches' per-tensor scalars (stream-ordered reuse)

    def _workspace(self, dev):
        ws = self._ws.get(dev)
        if ws is None:
            nb = int(_lib.load().msha_adam_workspace_size())
            ws = self._ws[dev] = torch.zeros(nb, dtype=torch.uint8, device=dev)
        return ws

    def _state_of(self, p):
        st = self.state[p]
        if not st:
            st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            return st
        # state loaded from elsewhere: the kernel reads 'step' (fp32) and the moments (the
        # parameter's dtype, contiguous) through device pointers
        stp = st["step"]
        if not (torch.is_tensor(stp) and stp.device == p.device and stp.dtype == torch.float32
                and stp.numel() == 1):
            st["step"] = torch.as_tensor(float(stp), dtype=torch.float32,
                                         device=p.device).reshape(())
        for k in ("exp_avg", "exp_avg_sq"):
            m = st[k]
            if m.device != p.device or m.dtype != p.dtype or not m.is_contiguous():
                st[k] = m.to(device=p.device, dtype=p.dtype).contiguous()
        return st

    def _group_of(self, p):
        for g in self.param_groups:
            if any(q is p for q in g["params"]):
                return g
        raise ValueError("parameter is not in this optimizer")

    @staticmethod
    def _check(p, g):
        _lib.require_cuda(p, g)
        if p.dtype not in _DT or g.dtype != p.dtype:
            raise TypeError(f"msha Adam: fp32 / bf16 parameters with same-dtype gradients "
                            f"(got {p.dtype} / {g.dtype})")
        if not (p.is_contiguous() and g.is_contiguous()):
            raise ValueError("msha Adam: contiguous parameters and gradients")

    def _desc(self, p, grad, drop_p=0.0, drop_seed=0):
        st = self._state_of(p)
        d = _lib.MshaAdamTensor()
        d.param, d.grad = p.data_ptr(), grad.data_ptr()
        d.exp_avg, d.exp_avg_sq = st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()
        d.step, d.n, d.dtype = st["step"].data_ptr(), p.numel(), _DT[p.dtype]
        d.drop_p, d.drop_seed, d.drop_offset = float(drop_p), int(drop_seed), 0
        return d

    def _launch(self, group, descs, dev):
        b1, b2 = group["betas"]
        for lo in range(0, len(descs), _lib.MAX_ADAM):
            part = descs[lo:lo + _lib.MAX_ADAM]
            arr = (_lib.MshaAdamTensor * len(part))(*part)
            _lib.call("msha_adam_step", len(part), ctypes.byref(arr), float(group["lr"]),
                      float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]),
                      self._workspace(dev).data_ptr(), _lib.stream_handle(dev))

    def _check_groups(self):
        # a loaded torch.optim.Adam state_dict may carry flags this kernel does not run
        for g in self.param_groups:
            bad = [k for k in ("amsgrad", "maximize", "differentiable") if g.get(k)]
            if bad:
                raise NotImplementedError(f"msha Adam: {', '.join(bad)} set in a parameter "
                                          "group (loaded state_dict?)")

    def load_state_dict(self, state_dict):
        # torch casts every state tensor but 'step' to the parameter's dtype; a replay
        # table's row_step is an int32 record (bf16 would lose it past 256 steps): it goes
        # round torch's loader
        ids = [i for g in state_dict["param_groups"] for i in g["params"]]
        params = [p for g in self.param_groups for p in g["params"]]
        kept = {}
        if len(ids) == len(params):  # (else torch raises below)
            kept = {i: st["row_step"] for i, st in state_dict["state"].items()
                    if isinstance(st, dict) and "row_step" in st}
        if kept:
            state_dict = dict(state_dict, state={
                i: ({k: v for k, v in st.items() if k != "row_step"} if i in kept else st)
                for i, st in state_dict["state"].items()})
        super().load_state_dict(state_dict)
        self._check_groups()
        for i, p in zip(ids, params):
            if i in kept:
                self.state[p]["row_step"] = torch.as_tensor(kept[i]).to(
                    device=p.device, dtype=torch.int32, copy=True)
            if getattr(p, "_msha_row_replay", False):
                p._msha_replay_hp = None  # the loaded group's values: those of its last launch

    @torch.no_grad()
    def step(self, closure=None):
        self._check_groups()
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            by_dev = {}
            for p in group["params"]:
                if row_optimizer_of(p) is self:
                    replay = getattr(p, "_msha_row_replay", False)
                    if not replay:
                        self._check_row_group(group)
                    rg = self.row_grad_of(p)  # several pending: merged once
                    if rg is not None:  # the touched rows' gradient: a lazy step over them
                        if p.grad is not None:
                            raise RuntimeError(
                                "msha Adam: a fuse_row_grad parameter has both a row gradient "
                                "and a .grad (it has another consumer besides its link loss): "
                                "do not register it")
                        _drop_row_grads(p)
                        if replay:
                            self._replay_step(group, p, rg)
                        else:
                            self._rows_step(group, p, rg)
                        continue
                    if replay and (p.grad is not None
                                   or getattr(p, "_msha_dropout_grad", None) is not None):
                        # a dense step of a replay table (a view or a cast of it was
                        # trained): every row is brought up to date first and takes the step
                        self.catch_up(p)
                        self.state[p]["row_step"].add_(1)
                stash = getattr(p, "_msha_dropout_grad", None)
                if stash is not None:  # fused: the dropout's output gradient + its mask
                    if p.grad is not None:
                        # a second consumer of the fused parameter put a gradient in .grad:
                        # the fused update would silently drop it
                        raise RuntimeError(
                            "msha Adam: a fuse_dropout_grad parameter also has a .grad (it has "
                            "another consumer besides its feature dropout): do not fuse it")
                    dout, drop_p, seed = stash
                    p._msha_dropout_grad = None
                    self._check(p, dout)
                    by_dev.setdefault(p.device, []).append(self._desc(p, dout, drop_p, seed))
                    continue
                if p.grad is None:
                    continue
                g = p.grad
                if g.is_sparse:
                    raise NotImplementedError("msha Adam: sparse gradients")
                self._check(p, g)
                by_dev.setdefault(p.device, []).append(self._desc(p, g))
            for dev, descs in by_dev.items():
                self._launch(group, descs, dev)
        return loss

    def zero_grad(self, set_to_none: bool = True):
        super().zero_grad(set_to_none)
        for group in self.param_groups:
            for p in group["params"]:
                if getattr(p, "_msha_dropout_grad", None) is not None:
                    p._msha_dropout_grad = None
                _drop_row_grads(p)

    # ------------------------------------------------- row-sparse table updates
    @staticmethod
    def _check_row_group(group):
        if group["weight_decay"] != 0:
            raise ValueError("msha Adam: a fuse_row_grad table needs weight_decay == 0 in its "
                             "parameter group (L2 decay makes the gradient dense; this "
                             "optimizer has no decoupled decay)")

    def fuse_row_grad(self, param, accumulate=False, replay=False):
        """Train the 2-D leaf table ``param`` at the cost of the rows a batch touches;
        returns ``param``.  ``functional.link_bce_loss``, ``link_distill_loss``,
        ``link_mlp_loss``, ``link_match_loss`` (with ``rows``) and ``sage_forward`` called on
        the table itself then hand their backward's ``functional.RowGrad`` (the touched rows
        of the batch and their fp32 gradient rows, bit for bit the dense gradient's) to this
        optimizer in place of ``param.grad``, which stays None: no (n, F) gradient is
        allocated.  ``step()`` runs ``msha_adam_rows_step`` over those rows: this
        optimizer's update with one global step count, for the touched rows only; the
        moments of the other rows are not decayed (``torch.optim.SparseAdam``'s rule with
        eps inside the bias correction).  A step that touches every row leaves the bits of
        the unregistered update.  One row gradient per step (a second backward before
        ``step()`` raises) unless ``accumulate`` is set: then up to four row gradients may
        arrive before ``step()`` (several losses on one table, or one backward of their sum),
        and ``step()`` first sums them in arrival order over the union of their rows
        (``functional.row_grad_union``: for fp32 the bits of accumulating the dense gradients).
        The group's ``weight_decay`` must be 0.  A view, a cast or an
        encoder's output of the table takes the dense path as before.  When a batch names
        every row (P in the millions on a 100k-row table) the list adds work and nothing is
        saved: the registered step may then be slower than the dense one
        (profiles/row_adam_ab).

        ``replay=True``: the dense optimizer's trajectory instead of the frozen-moment one,
        and the group's ``weight_decay`` may be non-zero (SGAE.py:79, train.py:207 train with
        5e-4).  ``step()`` runs ``msha_adam_rows_replay``: a stepped row first takes the
        steps it missed -- zero gradient plus ``weight_decay * p``, each with its own bias
        corrections -- and then this step, between one read and one write of the row.  The
        state gains ``row_step`` (int32, one per row, part of ``state_dict()``; a loaded
        state without it means every row is current).  Rows that no batch names are stale in
        memory until they are next read: the five losses above catch up the rows they read
        (``catch_up(param, plan)``, one more launch, capturable); any other reader calls
        ``catch_up(param)`` first.  After it the table and both moments hold the bits of the
        unregistered run.  All replayed steps use one set of (lr, betas, eps, weight_decay):
        when the group's values change, the next ``step()`` / ``catch_up()`` first brings
        every row up to date under the old ones (one pass over the table and one readback of
        the step count), so a scheduler that changes lr every step makes this path dense."""
        group = self._group_of(param)  # must be ours
        if param.dim() != 2 or not param.is_leaf:
            raise ValueError("msha Adam: fuse_row_grad takes a 2-D leaf table, got "
                             f"{tuple(param.shape)}")
        if not replay:
            self._check_row_group(group)
        param._msha_row_adam = weakref.ref(self)
        param._msha_row_accumulate = bool(accumulate)
        param._msha_row_replay = bool(replay)
        param._msha_replay_hp = None
        if replay:
            self._replay_state(param)
        return param

    def stash_row_grad(self, param, row_grad):
        """Called from a loss's backward: keep the table's ``functional.RowGrad`` for
        ``step()`` in place of ``param.grad``."""
        pending = getattr(param, "_msha_row_grads", None) or []
        if pending and not getattr(param, "_msha_row_accumulate", False):
            raise RuntimeError("msha Adam: a fuse_row_grad table got a second backward before "
                               "step(); one row gradient per step (do not register a table "
                               "that two losses share, or register it with accumulate=True)")
        if len(pending) >= MAX_ROW_GRADS:
            raise RuntimeError(f"msha Adam: a fuse_row_grad(accumulate=True) table takes at most "
                               f"{MAX_ROW_GRADS} row gradients per step")
        if tuple(row_grad.shape) != tuple(param.shape):
            raise ValueError("msha Adam: the row gradient is not of this table's shape")
        param._msha_row_grads = pending + [row_grad]
        param._msha_row_merged = None

    def row_grad_of(self, param):
        """The pending ``functional.RowGrad`` of a registered table, or None; with several
        pending (``accumulate=True``) their sum, formed once and kept until ``step()`` or
        ``zero_grad()``."""
        pending = getattr(param, "_msha_row_grads", None)
        if not pending:
            return None
        if len(pending) == 1:
            return pending[0]
        if getattr(param, "_msha_row_merged", None) is None:
            from .functional import row_grad_union

            param._msha_row_merged = row_grad_union(pending)
        return param._msha_row_merged

    def _rows_step(self, group, p, rg):
        _lib.require_cuda(p, rg.values)
        if p.dtype not in _DT or not p.is_contiguous():
            raise TypeError("msha Adam: a fuse_row_grad table is a contiguous fp32 / bf16 "
                            f"parameter (got {p.dtype})")
        st = self._state_of(p)
        b1, b2 = group["betas"]
        _lib.call("msha_adam_rows_step", p.shape[0], p.shape[1], _DT[p.dtype], p.data_ptr(),
                  st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), st["step"].data_ptr(),
                  rg.rows.data_ptr(), rg.n_rows.data_ptr(), rg.rows.numel(),
                  rg.values.data_ptr(), float(group["lr"]), float(b1), float(b2),
                  float(group["eps"]), _lib.stream_handle(p.device))

    # ------------------------------------------ row-sparse updates, missed steps replayed
    def _replay_state(self, p):
        """The state of a replay table with its ``row_step``; without one (fresh state, or
        a loaded state_dict that has none) every row is current: the step count."""
        st = self._state_of(p)
        rs = st.get("row_step")
        n = p.shape[0]
        if rs is None:
            st["row_step"] = st["step"].to(torch.int32).expand(n).contiguous()
        elif (rs.dtype != torch.int32 or rs.device != p.device or rs.shape != (n,)
              or not rs.is_contiguous()):
            if rs.numel() != n:
                raise ValueError(f"msha Adam: row_step has {rs.numel()} entries, the table "
                                 f"{n} rows")
            st["row_step"] = rs.to(device=p.device, dtype=torch.int32).reshape(n).contiguous()
        return st

    @staticmethod
    def _hyper(group):
        b1, b2 = group["betas"]
        return (float(group["lr"]), float(b1), float(b2), float(group["eps"]),
                float(group["weight_decay"]))

    def _replay_launch(self, p, hyper, rows, n_rows, cap, vals, max_steps):
        if p.dtype not in _DT or not p.is_contiguous():
            raise TypeError("msha Adam: a fuse_row_grad table is a contiguous fp32 / bf16 "
                            f"parameter (got {p.dtype})")
        st = self._replay_state(p)
        _lib.call("msha_adam_rows_replay", p.shape[0], p.shape[1], _DT[p.dtype], p.data_ptr(),
                  st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), st["step"].data_ptr(),
                  st["row_step"].data_ptr(), _lib.ptr(rows), _lib.ptr(n_rows), cap,
                  _lib.ptr(vals), int(max_steps), *hyper, _lib.stream_handle(p.device))

    def _flush(self, p, hyper, chunk=None):
        """Every row of ``p`` up to the present under ``hyper``: ceil(T / chunk) launches of
        at most ``chunk`` replayed steps per row (one readback, of the step count)."""
        chunk = FLUSH_CHUNK if chunk is None else int(chunk)
        if chunk < 1:
            raise ValueError(f"msha Adam: chunk must be at least 1, got {chunk}")
        T = int(self._replay_state(p)["step"].item())
        for _ in range(-(-T // chunk)):
            self._replay_launch(p, hyper, None, None, p.shape[0], None, min(chunk, _ALL_STEPS))

    def _replay_hyper(self, group, p):
        """The group's hyperparameters; when they differ from those of the table's last
        launch, every row is first brought up to date under the old ones."""
        hyper = self._hyper(group)
        last = getattr(p, "_msha_replay_hp", None)
        if last is not None and last != hyper:
            self._flush(p, last)
        p._msha_replay_hp = hyper
        return hyper

    def _replay_step(self, group, p, rg):
        _lib.require_cuda(p, rg.values)
        # (a row behind by any number of steps must reach the present to take its gradient)
        self._replay_launch(p, self._replay_hyper(group, p), rg.rows, rg.n_rows,
                            rg.rows.numel(), rg.values, _ALL_STEPS)

    def _replay_table(self, param):
        if row_optimizer_of(param) is not self or not getattr(param, "_msha_row_replay", False):
            raise ValueError("msha Adam: not a table registered with "
                             "fuse_row_grad(replay=True) on this optimizer")
        return self._group_of(param)

    def catch_up(self, param, rows=None, chunk=None):
        """Bring rows of a ``fuse_row_grad(replay=True)`` table up to the present step, so
        that they can be read.  ``rows``: a ``functional.PairPlan`` (its ``plan_rows``) or a
        ``(rows, n_rows)`` pair of distinct int32 row ids and their device count -- one
        launch, nothing read back, capturable.  ``rows=None``: every row, the flush before
        evaluation, ``topk_inner`` / ``rank_inner`` / ``score_pairs``, indexing, or a
        checkpoint meant for another optimizer; it reads the step count T back once and
        issues ceil(T / chunk) launches of at most ``chunk`` (default ``FLUSH_CHUNK`` = 1024)
        replayed steps per row, so no single launch is unbounded; not meant to be captured.
        Rows that are current are not touched; calling it twice changes nothing."""
        group = self._replay_table(param)
        _lib.require_cuda(param)
        hyper = self._replay_hyper(group, param)
        if rows is None:
            self._flush(param, hyper, chunk)
            return
        from .functional import PairPlan, plan_rows

        rows, n_rows = plan_rows(rows) if isinstance(rows, PairPlan) else rows
        if rows.dtype != torch.int32 or n_rows.dtype != torch.int32:
            raise TypeError("msha Adam: catch_up takes int32 rows and an int32 device count "
                            "(plan_rows)")
        _lib.require_cuda(rows, n_rows)
        if rows.numel():
            self._replay_launch(param, hyper, rows, n_rows, rows.numel(), None, _ALL_STEPS)

    def stale_rows(self, param):
        """The number of rows of a replay table that are behind the step count (a device
        int64 scalar, a plain torch expression)."""
        self._replay_table(param)
        st = self._replay_state(param)
        return (st["row_step"] < st["step"].to(torch.int32)).sum()

    # ---------------------------------------------- fused dropout-backward updates
    def fuse_dropout_grad(self, param):
        """Update ``param`` inside its feature dropout's backward (functional.feature_dropout
        checks for this registration); returns ``param``."""
        self._group_of(param)  # must be ours
        param._msha_fused_adam = weakref.ref(self)
        return param

    def stash_dropout_grad(self, param, dout, p: float, seed: int):
        """Called from the feature dropout's backward: keep the dropout's output gradient
        ``dout`` and its mask (p, seed) for ``step()`` in place of ``param.grad``."""
        if getattr(param, "_msha_dropout_grad", None) is not None:
            raise RuntimeError("msha Adam: a fused parameter got a second backward before "
                               "step(); gradient accumulation needs its .grad (do not fuse)")
        dout = dout.contiguous()
        self._check(param, dout)
        param._msha_dropout_grad = (dout, float(p), int(seed))


def _drop_row_grads(param):
    if getattr(param, "_msha_row_grads", None):
        param._msha_row_grads = None
        param._msha_row_merged = None


def row_optimizer_of(param):
    """The msha Adam registered by ``fuse_row_grad`` for ``param`` (or None)."""
    ref = getattr(param, "_msha_row_adam", None)
    return ref() if ref is not None else None


def fused_optimizer_of(param):
    """The msha Adam registered by ``fuse_dropout_grad`` for ``param`` (or None)."""
    ref = getattr(param, "_msha_fused_adam", None)
    return ref() if ref is not None else None
