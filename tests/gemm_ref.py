"""Inputs of the exact layout sweep of the tiled GEMMs (csrc/gemm.hip, csrc/gemm_bf16.hip).

TEST INFRASTRUCTURE ONLY.  Three things live here, all host-side numpy:

``View`` / ``build_view``  an operand of a requested shape, strides and base misalignment as
    a window into a larger flat buffer pre-filled with NaN -- before the window, after it and
    in the pitch padding between its lines -- so an unmasked out-of-range read turns the
    product NaN.  ``out_view`` is the same for an output with ``ldc >= N``; ``outside`` is the
    mask of the buffer the kernel must leave alone.
case tables  ``F32_CASES``, ``BF16_CASES``, ``HO_CASES``, ``WGRAD_CASES``: one dict per case.
    Operands are small integers (|x| <= 8; |x| <= 2 for the head-outer terms), so every
    product and partial sum is an integer below 2^24 and fp32 / bf16 MFMA accumulation is
    exact in any order: the tests assert bit equality with the fp64 product
    (tests/test_gemm_host.py checks the bound over the tables).
``predict_f32`` / ``predict_bf16``  the documented layout rules (include/msha_gnn.h,
    msha_gemm_f32_loader / msha_gemm_bf16), restated from the header's wording: the loader
    code each case must take.  Each case also names the loader it was written to reach
    (``loader``), and the host test holds the two together.
"""
import zlib

import numpy as np

# MSHA_GEMM_LOADER_* of include/msha_gnn.h
SCALAR, BNF, AK, VEC = 0, 1, 2, 4
F32_LOADERS = {SCALAR, VEC, VEC | BNF, VEC | AK, VEC | AK | BNF}
BF16_LOADERS = {VEC, VEC | BNF, VEC | AK, VEC | AK | BNF}
GUARD = 16      # NaN elements before and after every window (64 B fp32, 32 B bf16)
EXACT = 2 ** 24  # integers below this are exact in fp32


class View:
    """A 2-D window into a flat buffer: ``buf`` (1-D float64 with NaN outside the window),
    element offset ``start`` of element (0, 0), element ``strides`` and ``shape``."""

    def __init__(self, buf, start, shape, strides):
        self.buf, self.start, self.shape, self.strides = buf, int(start), tuple(shape), tuple(strides)

    def index(self):
        r, c = np.meshgrid(np.arange(self.shape[0]), np.arange(self.shape[1]), indexing="ij")
        return self.start + r * self.strides[0] + c * self.strides[1]

    def values(self):
        return self.buf[self.index()]

    def misalign(self, itemsize):
        """Bytes of the window's base past a 16-byte boundary (the buffer itself is aligned)."""
        return (self.start * itemsize) % 16

    def outside(self):
        """Mask over ``buf`` of everything that is not an element of the window."""
        m = np.ones(self.buf.shape, bool)
        m[np.unique(self.index())] = False
        return m


def spec(order, off=0, pitch=None, step=1):
    """Operand layout: ``order`` 'r' (last index contiguous) or 'c' (first index contiguous),
    base ``off`` elements past an aligned address, ``pitch`` elements between lines (default:
    the line rounded up to a multiple of 8, plus 8 of padding), ``step`` the stride along the
    line (2: no unit stride)."""
    return dict(order=order, off=off, pitch=pitch, step=step)


ZERO_ROW = dict(order="zero", off=0, pitch=0, step=0)  # the (1, B) ones row of stride (0, 0)


def build_view(vals, sp):
    """``vals`` (R, C) laid out as ``sp`` asks, NaN everywhere else."""
    vals = np.asarray(vals, np.float64)
    R, C = vals.shape
    if sp["order"] == "zero":
        assert R == 1 and np.all(vals == vals[0, 0])
        buf = np.full(2 * GUARD + 1, np.nan)
        buf[GUARD] = vals[0, 0]
        return View(buf, GUARD, (R, C), (0, 0))
    lines, length = (R, C) if sp["order"] == "r" else (C, R)
    step = sp["step"]
    span = (length - 1) * step + 1
    pitch = sp["pitch"] if sp["pitch"] is not None else (span + 7) // 8 * 8 + 8
    assert pitch >= span
    start = GUARD + sp["off"]
    buf = np.full(start + (lines - 1) * pitch + span + GUARD, np.nan)
    strides = (pitch, step) if sp["order"] == "r" else (step, pitch)
    v = View(buf, start, (R, C), strides)
    buf[v.index()] = vals
    return v


def out_view(M, N, ldc, off=0, fill=None):
    """Output window (M, N) of pitch ``ldc`` in a NaN buffer; ``fill`` (M, N): its prior
    content (accumulate), else NaN like the rest."""
    assert ldc >= N
    start = GUARD + off
    buf = np.full(start + (M - 1) * ldc + N + GUARD, np.nan)
    v = View(buf, start, (M, N), (ldc, 1))
    if fill is not None:
        buf[v.index()] = fill
    return v


def ints(name, shape, bound):
    """Integers in [-bound, bound] from an rng seeded by the case name and the shape."""
    rng = np.random.default_rng(zlib.crc32(f"{name}{shape}{bound}".encode()))
    return rng.integers(-bound, bound + 1, shape).astype(np.float64)


# ------------------------------------------------------------------ the documented rules
def predict_f32(M, N, K, a_mis, sAm, sAk, b_mis, sBk, sBn):
    """msha_gemm_f32_loader as include/msha_gnn.h words it.  ``a_mis`` / ``b_mis``: bytes
    of the base past a 16-byte boundary."""
    if sAk == 1:                      # A's k is tried before its m
        a_ok, ak = a_mis == 0 and sAm % 4 == 0 and K % 4 == 0, True
    elif sAm == 1:
        a_ok, ak = a_mis == 0 and sAk % 4 == 0 and M % 4 == 0, False
    else:
        a_ok, ak = False, False
    if sBn == 1:                      # B's n is tried before its k
        b_ok, bn = b_mis == 0 and sBk % 4 == 0 and N % 4 == 0, True
    elif sBk == 1:
        b_ok, bn = b_mis == 0 and sBn % 4 == 0 and K % 4 == 0, False
    else:
        b_ok, bn = False, False
    if not (a_ok and b_ok):
        return SCALAR
    return VEC | (AK if ak else 0) | (BNF if bn else 0)


def _bf16_operand(mis, srow, sk, rows, K):
    """One operand of msha_gemm_bf16: True (k contiguous), False (row contiguous), None."""
    if mis != 0:
        return None
    if sk == 1 and srow % 8 == 0 and K % 8 == 0:
        return True
    if srow == 1 and sk % 8 == 0 and rows % 8 == 0:
        return False
    return None


def predict_bf16(M, N, K, a_mis, sAm, sAk, b_mis, sBk, sBn):
    a = _bf16_operand(a_mis, sAm, sAk, M, K)
    b = _bf16_operand(b_mis, sBn, sBk, N, K)
    if a is None or b is None:
        return -1
    return VEC | (AK if a else 0) | (0 if b else BNF)


def case_strides(c, itemsize):
    """(a_mis, sAm, sAk, b_mis, sBk, sBn) of a case, from the views the builder makes."""
    a = build_view(np.zeros((c["M"], c["K"])) if c["a"]["order"] != "zero"
                   else np.ones((c["M"], c["K"])), c["a"])
    b = build_view(np.zeros((c["K"], c["N"])), c["b"])
    return (a.misalign(itemsize), a.strides[0], a.strides[1],
            b.misalign(itemsize), b.strides[0], b.strides[1])


# ------------------------------------------------------------------------- case tables
def _lay(code):
    """(A order, B order) of a vector loader code."""
    return ("r" if code & AK else "c"), ("r" if code & BNF else "c")


def _ldc(M, N, K):
    """Half the cases store into a padded output (ldc > N, a multiple of 4: vector stores),
    the other half into a dense one."""
    return N if ((M + N + K) // 4) % 2 == 0 else (N + 3) // 4 * 4 + 4


def _case(name, M, N, K, a, b, loader, splits=1, accumulate=False, ldc=None, coff=0, **kw):
    return dict(name=name, M=M, N=N, K=K, a=a, b=b, loader=loader, splits=splits,
                accumulate=accumulate, ldc=_ldc(M, N, K) if ldc is None else ldc, coff=coff, **kw)


def _f32_cases():
    cs = []
    # the four 16-byte loaders over ragged M / N / K tiles (tile 128 x 128 x 32)
    for code in (VEC | AK | BNF, VEC | AK, VEC | BNF, VEC):
        ao, bo = _lay(code)
        for M in (4, 128, 132, 260):
            for N in (4, 128, 132):
                for K in (4, 32, 36, 100):
                    cs.append(_case(f"vec{code}-{M}x{N}x{K}", M, N, K, spec(ao), spec(bo), code))
    # the scalar loader, by each condition alone (everything else as a vector loader wants)
    M, N, K = 132, 132, 36
    s = lambda name, M, N, K, a, b, **kw: cs.append(_case("edge-" + name, M, N, K, a, b,  # noqa: E731
                                                         SCALAR, **kw))
    s("a-base+1", M, N, K, spec("r", off=1), spec("r"))
    s("b-base+1", M, N, K, spec("r"), spec("r", off=1))
    s("at-base+1", M, N, K, spec("c", off=1), spec("c"))
    for k in (1, 3, 31, 33):
        s(f"K{k}-a-kcontig", M, N, k, spec("r"), spec("r"))
    for k in (3, 33):
        s(f"K{k}-b-kcontig", M, N, k, spec("c"), spec("c"))
    s("N130-b-ncontig", M, 130, K, spec("r"), spec("r"))
    s("M130-a-mcontig", 130, N, K, spec("c"), spec("r"))
    s("a-pitch37", M, N, K, spec("r", pitch=37), spec("r"))
    s("b-pitch133", M, N, K, spec("r"), spec("r", pitch=133))
    s("at-pitch134", M, N, K, spec("c", pitch=134), spec("r"))
    s("bt-pitch38", M, N, K, spec("r"), spec("c", pitch=38))
    s("a-step2", M, N, K, spec("r", step=2), spec("r"))
    s("b-step2", M, N, K, spec("r"), spec("r", step=2))
    s("ones-row-N3", 1, 3, 300, ZERO_ROW, spec("r", pitch=3), ldc=3)
    s("ones-row-N64", 1, 64, 300, ZERO_ROW, spec("r", pitch=64), ldc=64)
    s("M1", 1, N, K, spec("r"), spec("r"))     # a vector loader: M is not A's contiguous extent
    cs[-1]["loader"] = VEC | AK | BNF
    s("M1-at", 1, N, K, spec("c"), spec("r"))
    s("N1", M, 1, K, spec("r"), spec("r"))
    s("N1-bt", M, 1, K, spec("r"), spec("c"))  # B k-contiguous: N is not its contiguous extent
    cs[-1]["loader"] = VEC | AK
    s("K1", M, N, 1, spec("r"), spec("r"))
    s("K1-at", M, N, 1, spec("c"), spec("r"))  # neither operand is loaded 4-along-k
    cs[-1]["loader"] = VEC | BNF
    s("M1N1K1", 1, 1, 1, spec("r"), spec("r"))
    # split-K: used < splits (K = 100: chunks of 32 -> 4 slabs), a ragged last chunk
    # (K = 5000 / 7 -> chunks of 736, the last 584), each also accumulating into C
    for acc in (False, True):
        t = "-acc" if acc else ""
        for sp_ in (2, 8):
            cs.append(_case(f"split{sp_}-K100{t}", 132, 132, 100, spec("r"), spec("r"),
                            VEC | AK | BNF, splits=sp_, accumulate=acc))
        cs.append(_case(f"split8-K100-scalar{t}", 130, 130, 100, spec("c"), spec("r"), SCALAR,
                        splits=8, accumulate=acc))
        cs.append(_case(f"split7-K5000{t}", 132, 132, 5000, spec("r"), spec("r"),
                        VEC | AK | BNF, splits=7, accumulate=acc))
        cs.append(_case(f"split7-K5000-wgrad{t}", 132, 132, 5000, spec("c"), spec("r"),
                        VEC | BNF, splits=7, accumulate=acc))
        cs.append(_case(f"split1{t}", 132, 132, 36, spec("r"), spec("c"), VEC | AK,
                        accumulate=acc))
    # store epilogue: odd ldc and a misaligned C take the scalar stores
    cs.append(_case("store-ldc135", 132, 132, 36, spec("r"), spec("r"), VEC | AK | BNF, ldc=135))
    cs.append(_case("store-c-base+1", 132, 132, 36, spec("r"), spec("r"), VEC | AK | BNF,
                    ldc=136, coff=1))
    cs.append(_case("store-c-base+1-N130", 132, 130, 36, spec("r"), spec("c"), VEC | AK,
                    ldc=131, coff=1))
    cs.append(_case("store-split-ldc135", 132, 132, 100, spec("r"), spec("r"), VEC | AK | BNF,
                    splits=2, ldc=135, coff=1))
    return cs


def _bf16_cases():
    cs = []
    for code in (VEC | AK | BNF, VEC | AK, VEC | BNF, VEC):
        ao, bo = _lay(code)
        kc = ao == "r" or bo == "c"  # an operand is k-contiguous: K a multiple of 8
        for M in ((4, 128, 132, 260) if ao == "r" else (8, 128, 136, 264)):
            for N in (8, 128, 136):
                for K in ((8, 32, 40, 104) if kc else (4, 32, 36, 100)):
                    for cbf in (False, True):
                        cs.append(_case(f"bf16-vec{code}-{M}x{N}x{K}-{'bf16' if cbf else 'f32'}",
                                        M, N, K, spec(ao), spec(bo), code, ldc=N, cbf=cbf))
    # split-K with used < splits (tile K = 64: K = 104 -> 2 slabs of 8, K = 200 -> 4 of 16)
    for cbf in (False, True):
        t = "bf16" if cbf else "f32"
        cs.append(_case(f"bf16-split8-K104-{t}", 136, 136, 104, spec("r"), spec("r"),
                        VEC | AK | BNF, splits=8, ldc=136, cbf=cbf))
        cs.append(_case(f"bf16-split16-K200-{t}", 136, 136, 200, spec("c"), spec("c"), VEC,
                        splits=16, ldc=136, cbf=cbf))
    return cs


def _bf16_refusals():
    """The documented refusals of msha_gemm_bf16 (loader -1, or N % 8 != 0)."""
    r = lambda name, M, N, K, a, b: _case("bf16-refuse-" + name, M, N, K, a, b, -1, ldc=(N + 7) // 8 * 8)  # noqa: E731
    return [
        # both operands pass (B k-contiguous: N is not its contiguous extent): C refuses
        dict(r("N30", 136, 30, 40, spec("r"), spec("c")), loader=VEC | AK),
        r("K30-a-kcontig", 264, 64, 30, spec("r"), spec("r")),   # matmul's dA at 30 recipients
        r("K36-b-kcontig", 136, 64, 36, spec("c"), spec("c")),
        r("M132-a-mcontig", 132, 64, 40, spec("c"), spec("r")),
        r("a-base+1", 136, 64, 40, spec("r", off=1), spec("r")),
        r("b-base+1", 136, 64, 40, spec("r"), spec("r", off=1)),
        r("a-pitch44", 136, 64, 40, spec("r", pitch=44), spec("r")),
        r("a-step2", 136, 64, 40, spec("r", step=2), spec("r")),
    ]


def _ho_cases():
    """gemm_head_outer: operand 0, dX = (dh + de (x) a [+ de2 (x) a2]) W^T, and operand 1,
    dW = X^T (dh + ...), at M = 517 rows; ``off``: the updated operand's base offset (the
    msha_add_head_outer fallback); ``W``: the width of the other factor."""
    cs = []
    for dt in ("f32", "bf16"):
        for H, F in (((1, 4), (3, 8), (2, 20)) if dt == "f32" else ((1, 8), (3, 8))):
            for operand in (0, 1):
                for two in (False, True):
                    cs.append(dict(name=f"ho-{dt}-op{operand}-{H}x{F}-{'two' if two else 'one'}",
                                   dt=dt, operand=operand, M=517, H=H, F=F, W=40, two=two, off=0))
    for operand in (0, 1):
        cs.append(dict(name=f"ho-f32-op{operand}-fallback", dt="f32", operand=operand, M=517,
                       H=3, F=8, W=40, two=True, off=1))
    return cs


# the resident weight-gradient kernels (skinny.hip) behind msha_gemm_f32: M = N = 128,
# A = X^T, splits = 16; K a multiple of the 16-row step, of 4 only, of neither
WGRAD_CASES = [dict(name=f"wgrad-K{K}-beta{int(acc)}", M=128, N=128, K=K, a=spec("c"),
                    b=spec("r"), splits=16, accumulate=acc, ldc=128, coff=0, loader=VEC | BNF)
               for K in (4096, 4099, 4100) for acc in (False, True)]

F32_CASES = _f32_cases()
BF16_CASES = _bf16_cases()
BF16_REFUSALS = _bf16_refusals()
HO_CASES = _ho_cases()


def case_operands(c):
    """(A view, B view, fp64 product) of a gemm case, from its name's seed."""
    if c["a"]["order"] == "zero":
        A = np.ones((c["M"], c["K"]))
    else:
        A = ints(c["name"] + "A", (c["M"], c["K"]), 8)
    B = ints(c["name"] + "B", (c["K"], c["N"]), 8)
    return build_view(A, c["a"]), build_view(B, c["b"]), A @ B


def case_prior(c):
    """C's content before an accumulating call (integers, |x| <= 8), else None."""
    return ints(c["name"] + "C", (c["M"], c["N"]), 8) if c["accumulate"] else None


def ho_operands(c):
    """Arrays of a head-outer case: dh, de, a, de2, a2, the other factor, the sum, the fp64
    product and the sum of absolute products."""
    M, H, F, Wd = c["M"], c["H"], c["F"], c["W"]
    D = H * F
    n = c["name"]
    dh = ints(n + "dh", (M, D), 8)
    de, a = ints(n + "de", (M, H), 2), ints(n + "a", (H, F), 2)
    de2 = ints(n + "de2", (M, H), 2) if c["two"] else None
    a2 = ints(n + "a2", (H, F), 2) if c["two"] else None
    tot = dh + np.repeat(de, F, 1) * a.reshape(-1)
    atot = np.abs(dh) + np.abs(np.repeat(de, F, 1) * a.reshape(-1))
    if c["two"]:
        tot = tot + np.repeat(de2, F, 1) * a2.reshape(-1)
        atot = atot + np.abs(np.repeat(de2, F, 1) * a2.reshape(-1))
    other = ints(n + "other", (Wd, D) if c["operand"] == 0 else (M, Wd), 8)
    if c["operand"] == 0:
        ref, absum = tot @ other.T, atot @ np.abs(other.T)
    else:
        ref, absum = other.T @ tot, np.abs(other.T) @ atot
    return dict(dh=dh, de=de, a=a, de2=de2, a2=a2, other=other, tot=tot, ref=ref, absum=absum)


# msha_project_scores on the tiled kernel: 256 < M < 1024 (neither small.hip nor the
# resident-W kernel); K = 30 takes the scalar loader (K % 4 != 0 with X k-contiguous)
PROJ_CASES = [dict(name=f"proj-K{K}-{H}x{F}-{sc}", M=300, K=K, H=H, F=F, scores=sc)
              for F in (4, 8, 16) for H in (1, 3) for K in (20, 30, 36)
              for sc in ("al", "ar", "both", "none")]


def proj_arrays(c):
    """X, W (|x| <= 8), al, ar and the output gradients dh, dl, dr (|x| <= 2) of a case."""
    M, K, H, F, n = c["M"], c["K"], c["H"], c["F"], c["name"]
    return dict(X=ints(n + "X", (M, K), 8), W=ints(n + "W", (K, H * F), 8),
                al=ints(n + "al", (H, F), 2), ar=ints(n + "ar", (H, F), 2),
                dh=ints(n + "dh", (M, H * F), 2), dl=ints(n + "dl", (M, H), 2),
                dr=ints(n + "dr", (M, H), 2))


def proj_abs_max(c):
    """The largest sum of absolute terms over every output and gradient of a case (all
    score terms present: the other configurations sum fewer)."""
    d = {k: np.abs(v) for k, v in proj_arrays(c).items()}
    M, H, F = c["M"], c["H"], c["F"]
    h = d["X"] @ d["W"]
    h3 = h.reshape(M, H, F)
    el = (h3 * d["al"]).sum(-1) + (h3 * d["ar"]).sum(-1)
    tot = d["dh"] + np.repeat(d["dl"], F, 1) * d["al"].reshape(-1) \
        + np.repeat(d["dr"], F, 1) * d["ar"].reshape(-1)
    dX, dW = tot @ d["W"].T, d["X"].T @ tot
    dal = np.einsum("mh,mhf->hf", d["dl"] + d["dr"], h3)
    return max(x.max() for x in (h, el, dX, dW, dal))
