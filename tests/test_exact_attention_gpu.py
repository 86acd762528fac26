"""-m gpu: the relation attention (every build of attn_batched_kernel, and attn_combine_batched_kernel) BIT FOR BIT against
the two-level softmax cases of tests/exact_attention_cases.py, whose result has no rounding freedom (the theorem in that
module's docstring; tests/test_exact_attention_cases.py proves on the CPU that the comparison bites).  Every case goes through
ops.relation_attention_batched -- one problem per launch, the mixed three-problem launch, the split launches -- at the ring
test's geometries, for f32 (one and two segments), bf16 and f16, the latter two with the f32 residual stream on and off, and is
compared with torch.equal.  Around everything the kernel may read lies NaN: a leak shows up as a NaN in the output.

A failure names the first wrong (query, head, column) and the keys selected there, with their tiles, segments and splits."""
import pytest
import torch

import exact_attention_cases as xa

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("combo", xa.COMBOS, ids=xa.combo_id)
def test_attention_is_exact(dev, combo):
    from mega.pytorch_amd import ops
    dt, variant, io_f32 = combo
    odt = xa.out_dtype(dt, io_f32)
    lib = ops._lib.load()
    bad, n, elems = [], 0, 0
    for name, geoms in xa.launches(variant):
        cases = [xa.checked_case(g, variant) for g in geoms]       # (a case that misses a condition is refused)
        for c in cases:
            assert lib.mega_relation_attention_splits(c.Nq, c.Nk, xa.G) == xa.splits(c.Nq, c.Nk)
            assert (c.nsplit > 1) == name.startswith("split")
        outs = ops.relation_attention_batched([xa.item_for(c, dt, io_f32, dev) for c in cases])
        torch.cuda.synchronize()
        for i, (c, out) in enumerate(zip(cases, outs)):
            n += 1
            elems += out.numel()
            assert out.dtype == odt
            msg = xa.describe_mismatch(c, out, xa.expected(c, odt), "%s/%s[%d]" % (xa.combo_id(combo), name, i))
            if msg is not None:
                bad.append(msg)
    print("%s: %d problems in %d launches, %d output elements compared, %d problems differ" % (
        xa.combo_id(combo), n, len(xa.launches(variant)), elems, len(bad)))
    assert not bad, "%d of %d problems differ from the exact result:\n%s" % (len(bad), n, "\n".join(bad[:6]))


def test_the_split_cases_split(dev):
    from mega.pytorch_amd import ops
    for g in xa.SPLIT:
        assert ops._lib.load().mega_relation_attention_splits(g[0], g[1], 16) > 1
