"""Element-wise check of one streaming product against fp64 recomputed from the operands exactly as the kernel read them.

The operands are read back from the workspace as stored (bf16 and fp32 values are exact in fp64), so nothing upstream of the product
contributes error and the bound per element follows from the product's own arithmetic alone:

    bound =  k_terms * 2^-23 * mag        fp32 accumulation of k_terms products in ANY order, mag = |A| @ |B| (+ |extra|).  The textbook
                                          bound is k * 2^-24 (Higham, Accuracy and Stability, section 3.1: |fl(x.y) - x.y| <= gamma_k |x|.|y|);
                                          the factor 2 covers an accumulator that does not round to nearest.  Partial-sum slabs, split K
                                          and K segments only reorder the same sum.
           + 2^-8 * |ref|                 a bf16 store (8 significant bits: unit roundoff 2^-8, reached just above a power of two)
           + 2^-16 * mag                  an fp32 operand fed to the bf16 matrix pipe as two bf16 planes with lo x lo dropped: hi carries 8
                                          bits, lo 8 more (csrc/tile_lane.h::split8 + csrc/tile_stream.hip::mm_presplit)

Nothing here is fitted to a measured error.  Works on CPU and GPU tensors alike (the GPU tests keep the fp64 products on the device).
"""
import torch

EPS_ACC = 2.0 ** -23       # per accumulated term
EPS_BF16 = 2.0 ** -8       # bf16 store
EPS_PLANES = 2.0 ** -16    # two-plane operand, lo x lo dropped


class ProductMismatch(AssertionError):
    pass


def product_ref(A, B, extra=None):
    """(ref, mag) = (A @ B + extra, |A| @ |B| + |extra|) in fp64; A, B broadcast as torch.matmul does (batched / per frame / per group)."""
    A, B = A.double(), B.double()
    ref, mag = A @ B, A.abs() @ B.abs()
    if extra is not None:
        extra = extra.double()
        ref, mag = ref + extra, mag + extra.abs()
    return ref, mag


def product_bound(ref, mag, *, out_bf16, k_terms, split_planes=False):
    bound = (float(k_terms) * EPS_ACC) * mag
    if out_bf16:
        bound = bound + EPS_BF16 * ref.abs()
    if split_planes:
        bound = bound + EPS_PLANES * mag
    return bound


def check_bound(got, ref, bound, name):
    """Every element of `got` within `bound` of `ref` (and finite); returns the worst err / bound.  An element whose bound is 0 (all of
    its terms are zero) must be exact."""
    got = got.double()
    if tuple(got.shape) != tuple(ref.shape):
        raise ProductMismatch(f"{name}: result shape {tuple(got.shape)} against reference {tuple(ref.shape)}")
    if not bool(torch.isfinite(got).all()):
        bad = (~torch.isfinite(got)).nonzero()
        raise ProductMismatch(f"{name}: {bad.shape[0]} non-finite elements, first at {tuple(int(i) for i in bad[0])}")
    err = (got - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if worst > 1.0:
        flat = int(ratio.reshape(-1).argmax())
        idx = []
        for n in reversed(ratio.shape):
            idx.append(flat % n)
            flat //= n
        idx = tuple(reversed(idx))
        nbad = int((ratio > 1.0).sum())
        raise ProductMismatch(f"{name}: worst element (frame / batch .., row, column) = {idx}: got {float(got[idx]):.9g}, fp64 {float(ref[idx]):.9g}, "
                              f"err / bound = {worst:.3g} (bound {float(bound[idx]):.3g}); {nbad} of {ratio.numel()} elements exceed their bound")
    return worst


def check_product(got, A, B, *, extra=None, out_bf16, k_terms, split_planes=False, name):
    """got == A @ B (+ extra) element by element within the derived bound (module docstring).  Raises ProductMismatch (an AssertionError)
    naming the product, the worst (frame, row, column), err / bound there and the count of elements over the bound; returns the worst
    err / bound so that the caller can record it."""
    ref, mag = product_ref(A, B, extra)
    return check_bound(got, ref, product_bound(ref, mag, out_bf16=out_bf16, k_terms=k_terms, split_planes=split_planes), name)


def check_untouched(region, sentinel, name="padding"):
    """Padding the kernel must not write still holds the sentinel (compared as stored: pass integer views for NaN-poisoned memory)."""
    bad = region != sentinel
    if bool(bad.any()):
        first = tuple(int(i) for i in bad.nonzero()[0])
        raise ProductMismatch(f"{name}: {int(bad.sum())} of {region.numel()} padding elements were written, first at {first}")
