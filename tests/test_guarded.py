"""tests/guarded.py against stand-in writers (no GPU, no library).

The writers below are plain Python, not project code: one correct, four with one footprint fault
each.  check() passes the first and names the region and the word for each of the others, which is
the evidence that the GPU tests built on the arenas fail on a footprint error."""
import numpy as np
import pytest

import guarded as G

N, BATCH = 256, 3


def _operands(bits):
    rng = np.random.default_rng(bits)
    q = 0xFFF00001 if bits == 32 else (1 << 62) - 57
    a = rng.integers(0, q, size=(BATCH, N), dtype=np.uint64).astype(G.dtype_of(bits))
    b = rng.integers(0, q, size=(BATCH, N), dtype=np.uint64).astype(G.dtype_of(bits))
    return a, b


def _arena(bits):
    a, b = _operands(bits)
    return G.HostArena(bits, G.guard_words(N), c=BATCH * N, a=a, b=b), a, b


def _whole(arena, name):
    """The writer's raw access: the arena's buffer from the operand's first word on, with the
    words before it reachable through negative offsets."""
    start, words = arena.spans[name]
    return arena.buf, start, words


def write_correct(arena):
    buf, start, words = _whole(arena, "c")
    buf[start:start + words] = (arena["a"] ^ arena["b"]) >> 2


def write_one_past_the_end(arena):
    write_correct(arena)
    buf, start, words = _whole(arena, "c")
    buf[start + words] = 5


def write_one_before_the_start(arena):
    write_correct(arena)
    buf, start, _ = _whole(arena, "c")
    buf[start - 1] = 6


def write_touches_an_input(arena):
    write_correct(arena)
    arena["b"][N + 7] ^= 1


def write_leaves_the_last_word(arena):
    write_correct(arena)
    buf, start, words = _whole(arena, "c")
    buf[start + words - 1] = arena.sentinel


@pytest.mark.parametrize("bits", (32, 64))
def test_layout(bits):
    arena, a, b = _arena(bits)
    wb = bits // 8
    assert arena.guard == G.GUARD_MIN == 8192
    assert G.guard_words(3 * 65536, 65536) == 3 * 65536 and G.guard_words(256) == 8192
    assert int(arena.sentinel) == (1 << bits) - 1
    ends = 0
    for name in ("c", "a", "b"):
        view = arena[name]
        start, words = arena.spans[name]
        assert view.dtype == G.dtype_of(bits) and view.size == words == BATCH * N
        assert view.ctypes.data % 16 == wb and view.ctypes.data == arena.addr(name)
        assert arena.guard <= start - ends < arena.guard + 4
        ends = start + words
    assert arena.total - ends >= arena.guard
    assert np.array_equal(arena.get("a", a.shape), a) and np.array_equal(arena.get("b", b.shape), b)
    assert (arena["c"] == arena.sentinel).all()
    # everything outside the operands holds the sentinel
    assert int((arena.buf != arena.sentinel).sum()) <= 2 * BATCH * N


@pytest.mark.parametrize("bits", (32, 64))
def test_correct_writer_passes(bits):
    arena, a, b = _arena(bits)
    write_correct(arena)
    arena.check()
    assert np.array_equal(arena.get("c", a.shape), (a ^ b) >> 2)


@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("writer,kind,operand,offset,value", [
    (write_one_past_the_end, "guard overwritten", "c", BATCH * N, 5),
    (write_one_before_the_start, "guard overwritten", "c", -1, 6),
    (write_touches_an_input, "input changed", "b", N + 7, None),
    (write_leaves_the_last_word, "output not written", "c", BATCH * N - 1, -1),
])
def test_each_fault_is_caught_and_located(writer, kind, operand, offset, value, bits):
    arena, a, b = _arena(bits)
    writer(arena)
    with pytest.raises(G.GuardError) as ei:
        arena.check()
    e = ei.value
    assert (e.kind, e.operand, e.offset) == (kind, operand, offset)
    if value is None:
        value = int(b.reshape(-1)[offset]) ^ 1
    assert e.value == (value if value >= 0 else (1 << bits) - 1)
    assert f"{operand}[{offset}]" in str(e)


def test_a_guard_word_between_two_operands_is_named_by_the_nearer_one():
    arena, _, _ = _arena(32)
    write_correct(arena)
    start_a = arena.spans["a"][0]
    arena.buf[start_a - 2] = 0               # two words before a, a whole guard after c
    with pytest.raises(G.GuardError) as ei:
        arena.check()
    assert (ei.value.kind, ei.value.operand, ei.value.offset) == ("guard overwritten", "a", -2)
    arena.buf[start_a - 2] = arena.sentinel
    arena.buf[arena.total - 1] = 0           # the last word of the last guard
    with pytest.raises(G.GuardError) as ei:
        arena.check()
    assert ei.value.operand == "b" and ei.value.offset >= BATCH * N + arena.guard - 1


def test_in_place_operands_follow_the_output_rule():
    a, b = _operands(64)
    arena = G.HostArena(64, G.guard_words(N), inplace=("a",), a=a, b=b)
    assert arena.outputs == ["a"] and list(arena.inputs) == ["b"]
    arena["a"][...] = arena["a"] >> 1        # out == in: a is written, b is not
    arena.check()
    arena["a"][5] = arena.sentinel
    with pytest.raises(G.GuardError) as ei:
        arena.check()
    assert (ei.value.kind, ei.value.operand, ei.value.offset) == ("output not written", "a", 5)
