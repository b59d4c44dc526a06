"""tests/stream_product_ref.py on the CPU: an honest emulation of a streaming kernel's arithmetic passes with room to spare, and each
of the mistakes such a kernel makes (a dropped token, a row from the neighbouring tile, a frame boundary off by one, a missing K segment,
an element off by two ulps) fails.  These are the conditions that make tests/test_stream_products_gpu.py mean something.

Emulation: bf16 operands (their products are exact in fp32), fp32 accumulation one term at a time in a SHUFFLED order (optionally in
slabs that are then added, as the split-K forms do), optionally a round-to-nearest-even bf16 store.

On the 0.5 mark: the accumulation part of the bound (k * 2^-23 * mag, twice the textbook k * 2^-24) is what the honest emulation must
stay below HALF of -- asserted on the fp32 result for every case.  With a bf16 store the whole ratio cannot stay below 0.5 over more than
a handful of elements: 2^-8 is exactly the unit roundoff of bf16, round-to-nearest reaches it just above every power of two
(1 + 2^-8 -> 1 has relative error 2^-8 / (1 + 2^-8)), so a correct store gets arbitrarily close to ratio 1.  There the test asserts
ratio <= 1 for the stored result and < 0.5 for the sum in front of the store."""
import pytest
import torch

from tests.stream_product_ref import ProductMismatch, check_product, check_untouched, product_ref, EPS_ACC


def _operands(M, K, N, seed, batch=()):
    g = torch.Generator().manual_seed(seed)
    A = (0.3 + 0.7 * torch.rand(*batch, M, K, generator=g)) * torch.randn(*batch, M, K, generator=g).sign()
    B = 0.6 * torch.randn(*batch, K, N, generator=g)
    return A.bfloat16().float(), B.bfloat16().float()


def _emulate(A, B, seed, slabs=1, skip=()):
    """fp32 accumulation of the bf16 products in a shuffled order; `slabs` partial sums added at the end; `skip`: contraction indices left out"""
    K = A.shape[-1]
    g = torch.Generator().manual_seed(seed)
    order = [k for k in torch.randperm(K, generator=g).tolist() if k not in skip]
    parts = []
    per = -(-len(order) // slabs)
    for s in range(slabs):
        acc = torch.zeros(*A.shape[:-1], B.shape[-1], dtype=torch.float32)
        for k in order[s * per:(s + 1) * per]:
            acc = acc + A[..., :, k:k + 1] * B[..., k:k + 1, :]          # (exact products, one fp32 rounding per add)
        parts.append(acc)
    acc = parts[0]
    for p in parts[1:]:
        acc = acc + p
    return acc


def _bf16(x):
    return x.bfloat16().float()


@pytest.mark.parametrize("K,slabs", [(8, 1), (140, 1), (384, 1), (1024, 1), (20000, 128)])
@pytest.mark.parametrize("out_bf16", [False, True])
def test_honest_emulation_passes_with_room(K, slabs, out_bf16):
    M, N = (8, 12) if K > 4096 else (24, 40)
    A, B = _operands(M, K, N, seed=K)
    acc = _emulate(A, B, seed=K + 1, slabs=slabs)
    r32 = check_product(acc, A, B, out_bf16=False, k_terms=K, name=f"K={K} fp32")
    assert r32 < 0.5, r32                              # the accumulation bound is not marginal
    if out_bf16:
        r16 = check_product(_bf16(acc), A, B, out_bf16=True, k_terms=K, name=f"K={K} bf16")
        assert r16 <= 1.0, r16                         # (module docstring: a correct bf16 store reaches its unit roundoff)


def test_split_plane_operand_passes_and_its_term_is_needed():
    """An fp32 operand as two bf16 planes with lo x lo dropped against a bf16 operand split the same way (tile_stream.hip::mm_presplit)."""
    g = torch.Generator().manual_seed(5)
    A = torch.randn(16, 32, generator=g)                                   # fp32 operand
    B = (0.5 * torch.randn(32, 64, generator=g)).bfloat16().float()
    ah = _bf16(A)
    al = _bf16(A - ah)
    got = _emulate(ah, B, 1) + _emulate(al, B, 2)
    assert check_product(got, A, B, out_bf16=False, k_terms=2 * 32, split_planes=True, name="planes") < 0.5
    with pytest.raises(ProductMismatch):                                   # one plane alone is 2^-9, not 2^-16
        check_product(_emulate(ah, B, 1), A, B, out_bf16=False, k_terms=32, split_planes=True, name="hi plane only")


def test_dropped_token_row_of_a_long_contraction_fails():
    """dWt-like: (128 x tokens) @ (tokens x 96) over 4 116 tokens, one token never added."""
    K = 4116
    A, B = _operands(32, K, 96, seed=3)
    good = _emulate(A, B, 9, slabs=16)
    assert check_product(good, A, B, out_bf16=False, k_terms=K, name="all tokens") < 0.5
    bad = _emulate(A, B, 9, slabs=16, skip=(2077,))
    with pytest.raises(ProductMismatch, match="dropped token"):
        check_product(bad, A, B, out_bf16=False, k_terms=K, name="dropped token")


@pytest.mark.parametrize("out_bf16", [False, True])
def test_output_row_replaced_by_its_neighbour_fails(out_bf16):
    A, B = _operands(48, 384, 64, seed=4)
    got = _emulate(A, B, 2)
    got[31] = got[32]                                  # the last row of a 32-row tile written from the next tile's first row
    got = _bf16(got) if out_bf16 else got
    with pytest.raises(ProductMismatch) as e:
        check_product(got, A, B, out_bf16=out_bf16, k_terms=384, name="row 31 <- row 32")
    assert "(31," in str(e.value) and "row 31 <- row 32" in str(e.value)          # (names the product and the row)


def test_single_element_off_fails():
    K = 140
    A, B = _operands(40, K, 48, seed=6)
    acc = _emulate(A, B, 3)
    ref, mag = product_ref(A, B)
    # bf16 store: two ulps of the stored value
    st = _bf16(acc)
    bits = st.view(torch.int32).clone()
    bits[17, 5] += 2 << 16
    with pytest.raises(ProductMismatch, match="1 of"):
        check_product(bits.view(torch.float32), A, B, out_bf16=True, k_terms=K, name="two ulps")
    # fp32 store: 4 k 2^-23 mag
    off = acc.clone()
    off[17, 5] += float(4 * K * EPS_ACC * mag[17, 5])
    with pytest.raises(ProductMismatch, match="1 of"):
        check_product(off, A, B, out_bf16=False, k_terms=K, name="four bounds")


def test_last_row_of_a_frame_with_the_next_frames_operand_fails():
    """per-frame product X[s] @ T[s]^T (the hop-2 logits, the dX latent segment): row N - 1 of frame 2 computed against T[3]."""
    S, N, K = 5, 20, 384
    A, B = _operands(N, K, 32, seed=8, batch=(S,))
    got = _emulate(A, B, 4)
    assert check_product(got, A, B, out_bf16=False, k_terms=K, name="frames") < 0.5
    got[2, N - 1] = _emulate(A[2, N - 1:], B[3], 4)[0]
    with pytest.raises(ProductMismatch) as e:
        check_product(got, A, B, out_bf16=False, k_terms=K, name="frame boundary")
    assert f"(2, {N - 1}," in str(e.value)


@pytest.mark.parametrize("missing", [0, 1, 2])
def test_missing_k_segment_fails(missing):
    """dX-like: three K segments (128 + 66 + the row-scale term); one of them never accumulated."""
    g = torch.Generator().manual_seed(12)
    A1, B1 = _operands(64, 128, 96, seed=20)
    A2, B2 = _operands(64, 66, 96, seed=21)
    rs = torch.randn(64, 1, generator=g)
    Xr = _bf16(0.5 * torch.randn(64, 96, generator=g))
    segs = [_emulate(A1, B1, 1), _emulate(A2, B2, 2), rs * Xr]
    A, B = torch.cat([A1, A2], 1), torch.cat([B1, B2], 0)
    full = _bf16(segs[0] + segs[1] + segs[2])
    assert check_product(full, A, B, extra=rs.double() * Xr.double(), out_bf16=True, k_terms=128 + 66 + 2, name="dX") <= 1.0
    part = _bf16(sum(s for i, s in enumerate(segs) if i != missing))
    with pytest.raises(ProductMismatch):
        check_product(part, A, B, extra=rs.double() * Xr.double(), out_bf16=True, k_terms=128 + 66 + 2, name="dX without a segment")


def test_non_finite_result_and_shape_mismatch_fail():
    A, B = _operands(8, 16, 8, seed=1)
    got = _emulate(A, B, 1)
    with pytest.raises(ProductMismatch, match="shape"):
        check_product(got[:7], A, B, out_bf16=False, k_terms=16, name="short")
    got[3, 2] = float("nan")
    with pytest.raises(ProductMismatch, match="non-finite"):
        check_product(got, A, B, out_bf16=False, k_terms=16, name="nan")


def test_zero_bound_elements_must_be_exact():
    A, B = _operands(8, 16, 8, seed=2)
    A[5] = 0.0                                          # a zero padding row: mag = 0 there
    got = _emulate(A, B, 1)
    assert check_product(got, A, B, out_bf16=True, k_terms=16, name="zero row") <= 1.0
    got[5, 0] = 1e-30
    with pytest.raises(ProductMismatch):
        check_product(got, A, B, out_bf16=True, k_terms=16, name="zero row written")


def test_untouched_padding():
    buf = torch.full((6, 8), -1, dtype=torch.int32)     # 0xFFFFFFFF: the poison of the test workspaces
    check_untouched(buf[:, 5:], -1)
    buf[4, 6] = 0
    with pytest.raises(ProductMismatch, match=r"first at \(4, 1\)"):
        check_untouched(buf[:, 5:], -1, "pad columns")
