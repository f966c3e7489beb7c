"""Every compiled form of the cached-attention kernels against the fp64-softmax oracle: one test per row of tests/attn_forms_util.py's
table, its id the kernel's template list -- decode<DC,RG,GQ,PG,WN> is the decode_scores_kernel / decode_pv_kernel pair,
extend<DC,GQ,PG,WN> is bfp_attention_extend_kernel.  Each form's own output meets the oracle on each row's own keys; the bit-for-bit
comparisons with the form that has one switch fewer only say WHERE a failure comes from.  The stale-LDS screen of
tests/test_gpu_window_stale_lds.py follows for the forms with every switch on, at every DC."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import attn_forms_util as U  # noqa: E402
from attn_forms_util import DEV, bits, check  # noqa: E402
from paged_util import assert_untouched  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
PATTERNS = (None, 0x00000000, 0xFFFFFFFF, 0x7FC00000, 0x3F800000, 0x00000001, 0x80000000)      # None: the run without the poison


def _against_the_oracle(c, out):
    """every non-empty row within window_util.check's bounds of the oracle on ITS keys; empty rows and rows behind counts[b] exact zeros"""
    assert np.isfinite(out).all()
    for b, ref in enumerate(U.reference(c)):
        rows = out[b * c.group:(b + 1) * c.group]
        m = c.queries(b)
        assert not rows[:, m:].any(), f"cache row {b}: output behind its {m} queries is not zero"
        if m:
            check(rows[:, :m], ref)


def _run(c, splits):
    import torch
    q, k, v = U.arrays(c)
    qt = torch.from_numpy(np.array(q)).to(DEV)
    cache = U.fill(c, k, v, c.lengths)
    out = U.attend(c, qt, cache, splits)
    again = U.attend(c, qt, cache, splits)
    assert torch.equal(bits(out), bits(again)), "equal inputs, different bits"
    _against_the_oracle(c, out.cpu().numpy())
    # ---- twins with one switch fewer: where a failure above comes from
    if c.paged:
        contig = U.fill(c, k, v, c.lengths, paged=False)
        assert torch.equal(bits(out), bits(U.attend(c, qt, contig, splits))), "paged differs from the contiguous cache"
        assert_untouched(cache)
    if c.group > 1:
        G = c.group
        rep = U.fill(c, np.repeat(k, G, 0), np.repeat(v, G, 0), U.repeated(c.lengths, G))
        assert torch.equal(bits(out), bits(U.attend(c, qt, rep, splits, group=1, rep=G))), "grouped differs from group 1 on the repeated cache"
        if c.paged:
            assert_untouched(rep)
    if c.window is not None:
        wide = U.attend(c, qt, cache, splits, window=c.L)
        assert torch.equal(bits(wide), bits(U.attend(c, qt, cache, splits, window=None))), "W >= L differs from window=None"


@pytest.mark.parametrize("c", U.CASES, ids=lambda c: c.id)
def test_form_vs_oracle(c):
    for splits in c.splits or (None,):
        _run(c, splits)


# ---- stale LDS: the forms with every switch on ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def poison():
    import torch
    so = ROOT / "tools" / "lds_poison" / "liblds_poison.so"
    if not so.exists():
        pytest.fail("tools/lds_poison/liblds_poison.so is not built (__graft_entry__.build())")
    lib = ctypes.CDLL(str(so))

    def fill(pattern):
        if pattern is None:
            return
        rc = lib.lds_poison(ctypes.c_uint(pattern), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, rc
    return fill


def _screen(poison, attend):
    import torch
    outs = []
    for p in PATTERNS:
        poison(p)
        outs.append(attend().clone())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(outs[0]).all()) and float(outs[0].abs().max()) > 0
    for p, o in zip(PATTERNS[1:], outs[1:]):
        assert torch.equal(bits(o), bits(outs[0])), f"output depends on stale LDS (pattern {p:#010x})"


@pytest.mark.parametrize("c", U.ALL_ON, ids=lambda c: c.id)
def test_stale_lds_every_switch_on(poison, c):
    import torch
    q, k, v = U.arrays(c)
    qt = torch.from_numpy(np.array(q)).to(DEV)
    cache = U.fill(c, k, v, c.lengths)
    _screen(poison, lambda: U.attend(c, qt, cache, 2 if c.kind == "decode" else None))
    _against_the_oracle(c, U.attend(c, qt, cache, 2 if c.kind == "decode" else None).cpu().numpy())

