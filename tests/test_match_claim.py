"""k_match near the end of a block: its lanes (1024 per 16 Ki-position
quarter) take positions from a workgroup counter, each with its first link
and its first 8 window bytes read when it is taken.  A mistake there shows as
a position skipped, stored twice or walked past the block end, so single
blocks are cut to lengths whose last quarter holds a number of positions
around the multiples of the workgroup size, and every output is compared with
the oracle byte for byte and decoded again.  Level 9 takes k_match<true>
(16-byte matchlen steps), level 1 the greedy parse over the same records."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BS = 65536
QUARTER = 16384
TAILS = (1, 1023, 1024, 1025, 2047, 2048, 2049, 3071, 3072, 3073)
SIZES = sorted({QUARTER * k + r for k in (0, 1, 3) for r in TAILS} | {16384, 32768, 65536})


@functools.lru_cache(maxsize=None)
def _data(J, level: int, kind: str) -> bytes:
    """One buffer per level and kind; the cases are slices of it."""
    if kind == "text":
        return J.corpus_text(6 * BS, seed=300 + level).tobytes()
    # runs over {0, 1, 255}: lanes finish at very uneven times
    rng = np.random.default_rng(11 + level)
    return bytes(np.repeat(rng.choice([0, 1, 255], 3000), rng.integers(1, 120, 3000)).astype(np.uint8))


def _check(engine, oracle, data: bytes, level: int, what: str) -> None:
    g, gs = engine.deflate_blocks(data, level=level)
    o, osz = oracle.deflate_blocks(data, level=level)
    assert gs == osz, f"{what}: block sizes differ"
    assert g == o, f"{what}: deflate output differs from the oracle"
    back, us, errs = engine.inflate_blocks(g, gs)
    assert not any(errs), f"{what}: inflate errors {errs}"
    assert back == data, f"{what}: round trip differs"


@pytest.mark.parametrize("kind", ["text", "runs"])
@pytest.mark.parametrize("level", [6, 9, 1])
def test_last_quarter_around_workgroup_multiples(engine, oracle, level, kind):
    buf = _data(engine, level, kind)
    assert len(buf) >= BS
    for n in SIZES:
        _check(engine, oracle, buf[:n], level, f"level {level} {kind} n={n}")


def test_five_blocks_and_a_partial(engine, oracle):
    """Full quarters, a partial last block, and a grid that is no multiple of
    32 (the XCD-ordered block mapping falls back to the plain one)."""
    buf = _data(engine, 6, "text")
    _check(engine, oracle, buf[:5 * BS + 2049], 6, "5 blocks + 2049")
