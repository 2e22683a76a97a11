"""Shared set-up of the paged-cache tests (tests/test_paged_ref.py,
tests/test_gpu_paged.py): B sequences of up to TMAX positions dealt over a pool
of pages in a fixed scrambled, interleaved order, with NaN wherever nothing may
be read and -1 in the table entries that no position needs."""
import torch

B, H, TMAX = 3, 2, 256
SPARE = 3                      # pages of the pool that no sequence gets
NAN = float("nan")


def deal(PS):
    """(table (B,MP) int64 with every entry assigned, P): the pages of a pool
    of P = B*MP + SPARE dealt round-robin over the sequences from a fixed
    permutation, so a sequence's pages are neither contiguous nor monotonic."""
    MP = TMAX // PS
    P = B * MP + SPARE
    perm = torch.randperm(P, generator=torch.Generator().manual_seed(900 + PS))
    table = perm[:B * MP].view(MP, B).t().contiguous()
    for b in range(B):         # scrambled: some page number goes down
        assert bool((table[b, 1:] < table[b, :-1]).any())
    return table, P


def trim(table, PS, upto):
    """The table with -1 in every entry that positions [0, upto[b]) do not need."""
    t = table.clone()
    for b, n in enumerate(upto):
        t[b, -(-n // PS):] = -1
    return t


def nan_pool(P, PS, C, device, dtype):
    return (torch.full((P, H, PS, C), NAN, device=device, dtype=dtype),
            torch.full((P, H, PS, C), NAN, device=device, dtype=dtype))


def paged(k_all, v_all, kv_lens, PS):
    """From full caches (B,H,TMAX,C): the gathered caches with NaN at and past
    each length, the pools that hold rows [0, kv_lens[b]) of sequence b in its
    pages and NaN everywhere else (unused pages, and the rows past a length
    inside its last page), and the trimmed table."""
    table, P = deal(PS)
    kg, vg = k_all.clone(), v_all.clone()
    for b, n in enumerate(kv_lens):
        kg[b, :, n:] = NAN
        vg[b, :, n:] = NAN
    kp, vp = nan_pool(P, PS, k_all.shape[3], k_all.device, k_all.dtype)
    for b, n in enumerate(kv_lens):
        for j in range(-(-n // PS)):
            kp[table[b, j]] = kg[b, :, j * PS:(j + 1) * PS]
            vp[table[b, j]] = vg[b, :, j * PS:(j + 1) * PS]
    return kg, vg, kp, vp, trim(table, PS, kv_lens), P


def gather(pool, table, PS):
    """The pool seen through the table as (B,H,MP*PS,C); NaN where the entry is -1."""
    Bn, MP = table.shape
    out = torch.full((Bn, pool.shape[1], MP * PS, pool.shape[3]), NAN, device=pool.device,
                     dtype=pool.dtype)
    for b in range(Bn):
        for j in range(MP):
            if table[b, j] >= 0:
                out[b, :, j * PS:(j + 1) * PS] = pool[table[b, j]]
    return out


def nan_equal(a, b):
    return torch.equal(torch.nan_to_num(a, nan=12345.0), torch.nan_to_num(b, nan=12345.0)) \
        and torch.equal(torch.isnan(a), torch.isnan(b))
