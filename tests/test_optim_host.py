"""Host side of the fused AdamW (modules/optim.py): the learning-rate schedule, the chunk-table builder, the ABI entries and
train_like.py's flags.  No GPU."""
import math

import numpy as np
import pytest
import torch

SHAPES = [(1,), (3,), (5, 7), (4097,), (64, 64), (2, 3, 3, 3, 3), (8192,)]


def test_lr_at_against_hand_computed_values():
    from modules.optim import lr_at
    base, warmup, total = 1e-3, 4, 12
    want = {0: 2.5e-4,                                              # base * 1 / 4
            3: 1e-3,                                                # base * 4 / 4: the warm-up ends at base
            4: 1e-3,                                                # cos(0) = 1
            8: 5e-4,                                                # cos(pi / 2) = 0: half way down
            11: 0.5e-3 * (1.0 - 0.9238795325112867)}               # cos(7 pi / 8) = -cos(pi / 8)
    for k, v in want.items():
        assert lr_at(k, base, 'cosine', warmup, total) == pytest.approx(v, rel=1e-12, abs=1e-18), k
    assert lr_at(8, base, 'cosine', warmup, total, lr_min=1e-5) == pytest.approx(1e-5 + 0.5 * 9.9e-4, rel=1e-12)
    assert lr_at(12, base, 'cosine', warmup, total, lr_min=1e-5) == pytest.approx(1e-5, rel=1e-9)      # the end of the cosine
    assert lr_at(0, base, 'cosine', 0, 1) == base                   # no warm-up, one step: max(1, total - warmup) guards the division
    for k in (0, 3, 4, 11, 1000):
        assert lr_at(k, base, 'constant', warmup, total, lr_min=1e-5) == base
    with pytest.raises(ValueError):
        lr_at(0, base, 'linear', warmup, total)


def _params():
    g = torch.Generator().manual_seed(0)
    return [torch.nn.Parameter(torch.randn(s, generator=g)) for s in SHAPES]


@pytest.mark.parametrize('late_idx', [(), (2, 4)])
def test_chunk_table_covers_every_element_once(late_idx):
    from modules import parallel
    from modules.optim import CHUNK, chunk_table
    ps = _params()
    late = [ps[i] for i in late_idx]
    tab = chunk_table(ps, late=late)
    assert tab.dtype == np.int64 and tab.ndim == 2 and tab.shape[1] == 3
    assert CHUNK == 4096 and tab[:, 2].max() <= CHUNK and tab[:, 2].min() >= 1
    n = sum(p.numel() for p in ps)
    # the flat offsets tile [0, n) exactly once, in order
    assert tab[0, 1] == 0 and np.array_equal(tab[1:, 1], tab[:-1, 1] + tab[:-1, 2]) and tab[-1, 1] + tab[-1, 2] == n
    # the offsets are those of the bucket's own layout (early parameters first, then the late ones) ...
    bucket = parallel.GradBucket(ps, late=late)
    assert [id(p) for p in bucket.params] == [id(p) for p in ps if all(p is not q for q in late)] + [id(p) for p in late]
    flat0 = bucket.flat.data_ptr()
    covered = {id(p): np.zeros(p.numel(), dtype=np.int64) for p in ps}
    for addr, off, cnt in tab.tolist():
        owner = [p for p in ps if p.data_ptr() <= addr < p.data_ptr() + 4 * p.numel()]
        assert len(owner) == 1
        p = owner[0]
        first = (addr - p.data_ptr()) // 4
        assert (addr - p.data_ptr()) % 4 == 0 and first + cnt <= p.numel()          # ... and no chunk straddles a parameter
        assert (p.grad.data_ptr() - flat0) // 4 + first == off                       # same element in the parameter and in the bucket
        covered[id(p)][first:first + cnt] += 1
    assert all((c == 1).all() for c in covered.values())
    assert len(tab) == sum(-(-p.numel() // CHUNK) for p in ps)


def test_chunk_table_skips_frozen_parameters():
    from modules.optim import chunk_table
    ps = _params()
    ps[3].requires_grad_(False)
    tab = chunk_table(ps)
    assert tab[:, 2].sum() == sum(p.numel() for p in ps if p.requires_grad)


def test_abi_has_the_optimizer_entries():
    from modules import Extension as X
    for name in ('mvx_optim_workspace_bytes', 'mvx_optim_adamw_step'):
        assert name in X.PROTOTYPES and hasattr(X.lib, name)
    assert X.ABI_VERSION == 10 and X.lib.mvx_abi_version() == 10
    ws = X.lib.mvx_optim_workspace_bytes(1 << 20)
    assert 0 < ws <= 2048 * 12 + 256 and ws % 8 == 0 and ws == X.lib.mvx_optim_workspace_bytes(1)      # a constant grid of <= 2048 workgroups
    # argument errors come back before any launch (no GPU here): null pointers, then a beta outside [0, 1)
    assert X.lib.mvx_optim_adamw_step(None, 1, None, None, None, 16, None, None, 1e-3, 0.9, 0.999, 1e-6, 0.01, 0.0, 1, None, 0, None) == -1
    a = [0x1000, 1, 0x2000, 0x3000, 0x4000, 16, None, 0x5000]
    assert X.lib.mvx_optim_adamw_step(*a, 1e-3, 1.0, 0.999, 1e-6, 0.01, 0.0, 1, 0x6000, 1 << 20, None) == -1
    assert X.lib.mvx_optim_adamw_step(*a, 1e-3, 0.9, 0.999, 1e-6, 0.01, math.nan, 1, 0x6000, 1 << 20, None) == -1
    assert X.lib.mvx_optim_adamw_step(*a, 1e-3, 0.9, 0.999, 1e-6, 0.01, 0.0, 1, 0x6000, 8, None) == -1          # workspace too small


def test_bucket_divide_false_keeps_sum_and_count():
    from modules import parallel
    ps = _params()
    bucket = parallel.GradBucket(ps)
    bucket.flat.fill_(6.0)
    bucket.all_reduce_mean(frames_local=3, divide=False)
    assert float(bucket.count_slot()) == 3.0 and bucket.count_slot().data_ptr() == bucket.flat.data_ptr() + 4 * bucket.flat.numel()
    assert bool((bucket.flat == 6.0).all())
    bucket.all_reduce_mean(frames_local=3)
    assert bool((bucket.flat == 2.0).all())
    with pytest.raises(AssertionError):
        bucket.all_reduce_mean(frames_total=3, divide=False)


def test_train_like_flags():
    import train_like
    a = train_like.parse_args(['/nowhere', '--optimizer', 'hip', '--clip-grad-norm', '10', '--lr-schedule', 'cosine',
                               '--warmup-steps', '5', '--lr-min', '1e-5'])
    assert a.optimizer == 'hip' and a.clip_grad_norm == 10.0 and a.lr_schedule == 'cosine' and a.warmup_steps == 5 and a.lr_min == 1e-5
    train_like.check_optimizer_args(a)
    d = train_like.parse_args(['/nowhere'])
    assert d.optimizer == 'torch' and d.clip_grad_norm == 0.0 and d.lr_schedule == 'constant'
    train_like.check_optimizer_args(d)
    # flags that only the HIP optimizer implements are refused with the torch one, by train() itself, before it touches a GPU
    for extra in (['--clip-grad-norm', '10'], ['--lr-schedule', 'cosine'], ['--warmup-steps', '3']):
        bad = train_like.parse_args(['/nowhere', '--optimizer', 'torch'] + extra)
        with pytest.raises(SystemExit, match='--optimizer hip'):
            train_like.train(bad)
