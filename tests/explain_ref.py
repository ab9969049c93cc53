"""The CPU statement of the attention explanation's two selections, shared by the explain
tests, over ragged segments (``ptr`` + per-slot values and ids) and over dense rows:

  ties   the slots whose value is within ``rtol`` of the segment's maximum:
         value >= max - rtol * |max| (fp32: the product rounded, then the difference);
         with rtol = 0 or a non-finite maximum, the slots equal to the maximum
  top-K  the K best slots under (value descending, id ascending)

Both compare values through the order-preserving uint32 image the library documents: -0.0
folded onto +0.0, +inf highest, every NaN below -inf and all NaNs equal; 0 is "nothing".
Written from those definitions in integer numpy; ``test_explain_host`` checks it against a
brute-force float statement on dense rows."""
import numpy as np

NAN_IMAGE = np.uint32(1)


def image(x):
    """uint32 image of fp32 values: unsigned order == the selection's value order."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).copy()
    nan = (b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    b[b == np.uint32(0x80000000)] = 0
    neg = (b & np.uint32(0x80000000)) != 0
    key = np.where(neg, ~b, b ^ np.uint32(0x80000000)).astype(np.uint32)
    key[nan] = NAN_IMAGE
    return key


def value(img):
    """fp32 value of an image (0: -inf, "nothing"; the NaN image: a NaN)."""
    img = np.asarray(img, np.uint32)
    hi = (img & np.uint32(0x80000000)) != 0
    bits = np.where(hi, img ^ np.uint32(0x80000000), ~img).astype(np.uint32)
    out = bits.view(np.float32).copy()
    out[img == 0] = -np.inf
    out[img == NAN_IMAGE] = np.nan
    return out


def threshold_images(mx, rtol):
    """Images of the tie thresholds of segments whose maxima have the images ``mx``."""
    mx = np.asarray(mx, np.uint32)
    v = value(mx)
    with np.errstate(all="ignore"):
        t = v - np.float32(rtol) * np.abs(v)  # fp32: the product rounded, then the difference
    exact = (mx <= NAN_IMAGE) | (rtol == 0) | ~np.isfinite(v)
    return np.where(exact, mx, image(t)).astype(np.uint32)


def _slots(ptr, x, ids):
    """(segment, image, id) of every slot in [ptr[0], ptr[-1]), slot order."""
    ptr = np.asarray(ptr, np.int64)
    lo, hi = int(ptr[0]), int(ptr[-1])
    seg = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    pos = np.arange(lo, hi) - ptr[seg]
    return ptr, seg, image(np.asarray(x)[lo:hi]), (pos if ids is None else np.asarray(ids)[lo:hi])


def segment_ties(ptr, x, ids=None, rtol=0.0):
    """(max_val fp32 (n_seg), n_tie int32 (n_seg), tie_ptr int32 (n_seg + 1), tie_idx
    int32): per segment the maximum and the ids of the tied slots in slot order.  ``x``: the
    per-slot values; ``ids`` None: the position in the segment."""
    ptr, seg, img, sid = _slots(ptr, x, ids)
    n_seg = len(ptr) - 1
    mx = np.zeros(n_seg, np.uint32)
    np.maximum.at(mx, seg, img)
    tie = img >= threshold_images(mx, rtol)[seg]
    n_tie = np.bincount(seg[tie], minlength=n_seg).astype(np.int32)
    tie_ptr = np.zeros(n_seg + 1, np.int32)
    np.cumsum(n_tie, out=tie_ptr[1:])
    return value(mx), n_tie, tie_ptr, sid[tie].astype(np.int32)


def segment_topk(ptr, x, k, ids=None):
    """(values fp32 (n_seg, k), ids int64 (n_seg, k)), best first, filler -inf / -1."""
    ptr, seg, img, sid = _slots(ptr, x, ids)
    n_seg = len(ptr) - 1
    key = (img.astype(np.uint64) << np.uint64(32)) | (~sid.astype(np.uint64)
                                                      & np.uint64(0xFFFFFFFF))
    o = np.lexsort((~key, seg))  # by segment, then key descending
    seg, key = seg[o], key[o]
    rank = np.arange(len(seg)) - (ptr[seg] - ptr[0])
    keep = rank < k
    vals = np.full((n_seg, k), -np.inf, np.float32)
    idx = np.full((n_seg, k), -1, np.int64)
    vals[seg[keep], rank[keep]] = value((key[keep] >> np.uint64(32)).astype(np.uint32))
    idx[seg[keep], rank[keep]] = (~key[keep] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    return vals, idx


def lists(tie_ptr, tie_idx):
    return [np.asarray(tie_idx[tie_ptr[s]:tie_ptr[s + 1]]) for s in range(len(tie_ptr) - 1)]


def dense_ties(A, rtol=0.0):
    """Tie sets of every row of a dense matrix: a list of index arrays."""
    A = np.ascontiguousarray(A, np.float32)
    n, m = A.shape
    _, _, tp, ti = segment_ties(np.arange(n + 1) * m, A.reshape(-1), None, rtol)
    return lists(tp, ti)


def dense_topk(A, k):
    A = np.ascontiguousarray(A, np.float32)
    n, m = A.shape
    return segment_topk(np.arange(n + 1) * m, A.reshape(-1), k)


def same_f32(a, b):
    """Bitwise equality of fp32 arrays, any NaN equal to any NaN."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb)
                and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def csr_of_dense(A):
    """(rowptr, col, vals) of the non-zero entries of a dense matrix, row-major."""
    A = np.asarray(A)
    r, c = np.nonzero(A)
    rowptr = np.zeros(A.shape[0] + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=A.shape[0]), out=rowptr[1:])
    return rowptr, c, A[r, c]
