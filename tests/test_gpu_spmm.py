"""GPU: rsa_spmm_csr (ops.spmm_csr) against its float64 referee (tests/spmm_referee.py) -- every element within the bound, two
runs bit-equal -- over the widths, the row lengths around the chunk size, the skewed row, the nullable arguments, the in-place
accumulation and a source table past 4 GiB."""
import pytest
import torch

import spmm_referee as sr

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module')
def ra():
    import recstudio_amd
    recstudio_amd._native.lib()
    torch.cuda.init()
    return recstudio_amd


def csr_from_degrees(deg, n_cols, seed, last_col_row=None):
    """A CSR with the given row lengths, random columns (duplicates happen) and random values, on the device."""
    g = torch.Generator().manual_seed(seed)
    deg = torch.as_tensor(deg, dtype=torch.int64)
    indptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(deg, 0)])
    nnz = int(indptr[-1])
    indices = torch.randint(0, n_cols, (nnz,), generator=g, dtype=torch.int32)
    if last_col_row is not None:
        indices[int(indptr[last_col_row + 1]) - 1] = n_cols - 1
    values = torch.randn(nnz, generator=g)
    return indptr.to(DEV), indices.to(DEV), values.to(DEV)


def dense_inputs(n_rows, n_cols, d, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n_cols, d, generator=g).to(DEV), (torch.rand(n_rows, generator=g) + 0.5).to(DEV),
            torch.randn(n_rows, d, generator=g).to(DEV))


def check(ra, indptr, indices, values, x, chunk, row_scale=None, acc=None, acc_scale=1.0, want_y=True):
    """One call (twice: bit-equal), every output within the bound of the referee.  -> (y, acc')."""
    plan = ra.ops.spmm_plan(indptr, chunk)
    ref = sr.referee(indptr, indices, values, x, row_scale=row_scale, acc=acc, acc_scale=acc_scale)
    R, d = indptr.numel() - 1, x.shape[1]
    outs = []
    for _ in range(2):
        y = torch.full((R, d), float('nan'), device=DEV) if want_y or acc is None else None
        a = None if acc is None else acc.clone()
        got = ra.ops.spmm_csr(indptr, indices, values, x, plan=plan, row_scale=row_scale, y=y, acc=a, acc_scale=acc_scale)
        assert got is (y if y is not None else a)
        outs.append((y, a))
    torch.cuda.synchronize()
    for one, two in zip(*outs):
        assert (one is None) == (two is None)
        if one is not None:
            assert torch.equal(one, two), 'two runs differ'
            assert bool(torch.isfinite(one).all())
    ry, racc = sr.bound_ratios(ref, outs[0][0], outs[0][1])
    print(f'spmm R={R} nnz={indices.numel()} d={d} chunk={chunk} split={plan.n_split} parts={plan.n_parts}: '
          f'|y - ref| / bound = {ry}, |acc - ref| / bound = {racc}')
    assert ry is None or ry <= 1.0
    assert racc is None or racc <= 1.0
    return outs[0]


@pytest.mark.parametrize('d', [4, 36, 64, 128, 256])
def test_random_multigraph_split_path(ra, d):
    """300 x 200, power-law row lengths (up to 200 edges), chunk 8: split rows of 2 to 26 pieces between the short ones."""
    g = torch.Generator().manual_seed(11)
    deg = (200.0 / torch.arange(1, 301, dtype=torch.float64)).ceil().long()[torch.randperm(300, generator=g)] + \
        torch.randint(0, 6, (300,), generator=g)
    indptr, indices, values = csr_from_degrees(deg, 200, seed=12, last_col_row=299)
    x, scale, acc = dense_inputs(300, 200, d, seed=13)
    assert int(deg.max()) > 5 * 8 and int((deg > 8).sum()) > 20 and int((deg <= 8).sum()) > 100
    check(ra, indptr, indices, values, x, 8, row_scale=scale, acc=acc, acc_scale=0.25)


@pytest.mark.parametrize('d', [4, 36, 64, 256])
def test_row_lengths_around_the_chunk(ra, d):
    """Empty rows, rows of 1, chunk - 1, chunk, chunk + 1 and 5 chunk + 3 edges, a row count (4 k + 1) that is no multiple of the
    rows per workgroup, an edge to the last column; 64-edge batches: 63, 64, 65 edges in one piece with chunk 70."""
    for chunk, deg in ((8, [0, 1, 7, 8, 9, 43, 0, 0, 1, 8, 9, 43, 2]), (70, [63, 64, 65, 0, 70, 71, 353, 1, 129])):
        assert len(deg) % 4 == 1
        indptr, indices, values = csr_from_degrees(deg, 50, seed=21 + chunk, last_col_row=len(deg) - 1)
        x, scale, acc = dense_inputs(len(deg), 50, d, seed=22)
        y, a = check(ra, indptr, indices, values, x, chunk, row_scale=scale, acc=acc, acc_scale=0.5)
        empty = (torch.as_tensor(deg) == 0).nonzero().view(-1).to(DEV)
        assert float(y[empty].abs().max()) == 0.0                       # an empty row is written, as zeros
        assert torch.equal(a[empty], 0.5 * acc[empty])


def test_one_row_owns_half_the_edges(ra):
    """The skew case: one row with 2^17 of 2^18 edges (256 pieces of the default chunk), the rest spread over 4095 rows."""
    g = torch.Generator().manual_seed(31)
    rest = torch.bincount(torch.randint(0, 4095, (1 << 17,), generator=g), minlength=4095)
    deg = torch.cat([rest[:1000], torch.tensor([1 << 17]), rest[1000:]])
    assert int(deg.sum()) == 1 << 18
    indptr, indices, values = csr_from_degrees(deg, 3000, seed=32)
    x, scale, acc = dense_inputs(4096, 3000, 64, seed=33)
    check(ra, indptr, indices, values, x, ra.ops.SPMM_CHUNK, row_scale=scale, acc=acc, acc_scale=0.25)
    check(ra, indptr, indices, values, x, 8, row_scale=scale)             # 16384 pieces for the one row


def test_nullable_arguments_and_in_place_accumulation(ra):
    deg = [0, 3, 20, 9, 1, 70, 8, 5, 33]
    indptr, indices, values = csr_from_degrees(deg, 40, seed=41)
    x, scale, acc = dense_inputs(len(deg), 40, 64, seed=42)
    y_full, _ = check(ra, indptr, indices, values, x, 8, row_scale=scale)
    y_ones, _ = check(ra, indptr, indices, None, x, 8)                                       # values and row_scale null
    assert not torch.equal(y_full, y_ones)
    check(ra, indptr, indices, None, x, 8, row_scale=scale)
    check(ra, indptr, indices, values, x, 8)
    # y null with the accumulation; acc_in aliases acc_out (ops.spmm_csr always accumulates in place)
    y, a = check(ra, indptr, indices, values, x, 8, row_scale=scale, acc=acc, acc_scale=1.0 / 3.0, want_y=False)
    assert y is None
    y2, a2 = check(ra, indptr, indices, values, x, 8, row_scale=scale, acc=acc, acc_scale=1.0 / 3.0)
    assert torch.equal(a, a2) and torch.equal(y2, y_full)                 # the product does not depend on what else is written
    # a plan of another matrix, an aliased output and a bad width are refused on the host
    plan = ra.ops.spmm_plan(indptr, 8)
    with pytest.raises(ValueError, match='plan was built'):
        ra.ops.spmm_csr(indptr[:-1], indices[:int(indptr[-2])], None, x, plan=plan)
    with pytest.raises(ValueError, match='alias'):
        sq = torch.zeros(len(deg), 64, device=DEV)
        ra.ops.spmm_csr(indptr, indices.clamp(max=len(deg) - 1), None, sq, plan=plan, y=sq)
    with pytest.raises(ValueError, match='multiple of 4'):
        ra.ops.spmm_csr(indptr, indices, None, torch.zeros(40, 6, device=DEV), plan=plan)


def test_source_table_past_4_gib(ra):
    """x of 2^24 + 8 rows at d = 64 is 4 GiB + 2 KiB: rows past byte offset 2^32 are reached only with 64-bit offsets."""
    n_cols, d = (1 << 24) + 8, 64
    x = torch.zeros(n_cols, d, device=DEV)
    g = torch.Generator().manual_seed(51)
    cols = torch.tensor([0, n_cols - 1, n_cols - 2, n_cols - 8, 1 << 23, (1 << 24) - 1, 1 << 24, 5], dtype=torch.int64)
    x[cols.to(DEV)] = torch.randn(len(cols), d, generator=g).to(DEV)
    # row 0: the last rows and row 0; row 1: empty; row 2: 19 edges (split with chunk 8) over all of them; row 3: the last row alone
    idx = torch.cat([cols[:4], cols[torch.randint(0, len(cols), (19,), generator=g)], cols[1:2]]).int().to(DEV)
    indptr = torch.tensor([0, 4, 4, 23, 24], dtype=torch.int64, device=DEV)
    values = torch.randn(24, generator=g).to(DEV)
    y, _ = check(ra, indptr, idx, values, x, 8)
    assert torch.equal(y[3], values[23] * x[n_cols - 1]) and float(y[3].abs().max()) > 0
