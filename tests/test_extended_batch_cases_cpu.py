"""The case list of the extended levels' batch and members tests (tests/extended_batch_cases.py), guarded without a GPU: every
expected stream is a valid stream of its item, the copy-in-front cases discriminate (a window that reaches in front of the
item gives other bytes), only the random data is stored, and the members rule at levels 4..6 gives files gzip reads."""
import gzip

import pytest

import extended_batch_cases as xc
import members_write_cases as mw


@pytest.mark.parametrize("P", xc.PACKETS)
@pytest.mark.parametrize("level", xc.LEVELS)
def test_every_expected_stream_inflates_to_its_item(oracle, level, P):
    items = xc.items(P)
    assert [len(d) for d in items[:len(xc.lengths(P))]] == xc.lengths(P)
    for fmt in xc.FORMATS:
        for d, want in zip(items, xc.expected_items(oracle, fmt, level, P)):
            assert xc.inflate(want, fmt) == d, (len(d), fmt)
    for d in xc.many_items():
        assert xc.inflate(xc.expected_item(oracle, d, xc.DEFLATE, level, 4096), xc.DEFLATE) == d
    assert len(xc.many_items()) == 700 and all(1 <= len(d) <= 6000 for d in xc.many_items())


@pytest.mark.parametrize("level", xc.LEVELS)
def test_the_copy_cases_discriminate(oracle, level):
    for name, X in xc.copy_cases():
        assert len(X) == xc.COPY
        alone = oracle.encode_packets(X, xc.DEFLATE, level)
        leaked = oracle.packet(X + X, level, len(X), len(X), True)        # the same bytes with a copy of themselves as their window
        assert xc.inflate(alone, xc.DEFLATE) == X
        assert leaked != alone, name
        assert len(leaked) < 128 and len(alone) > 2000, (name, len(leaked), len(alone))   # a few long matches against thousands of bytes
        if name == "random":
            assert len(alone) == xc.COPY + 5                                 # one stored block


@pytest.mark.parametrize("level", xc.LEVELS)
def test_only_the_random_data_is_stored(oracle, level):
    for P in xc.PACKETS:
        raw = xc.expected_items(oracle, xc.DEFLATE, level, P)
        for i, (d, s) in enumerate(zip(xc.items(P), raw)):
            if len(d) >= 64:                                               # (below that a dynamic block's header alone outweighs the bytes)
                assert xc.stored_blocks_only(s) == (i in xc.random_items(P)), (i, len(d))
    for name, X in xc.copy_cases():
        file, offsets, stored = mw.expected(oracle, X * 3, level, xc.COPY, mw.PACKET, True)
        assert len(offsets) == 4 and gzip.decompress(file) == X * 3
        for at, size in mw.members_of(file[:offsets[-1]]):                 # (the encoder's own stored block is as short as the level-0 stream)
            assert xc.stored_blocks_only(file[at + 18:at + size - 8]) == (name == "random"), name


@pytest.mark.parametrize("level", xc.LEVELS)
def test_the_members_rule_at_the_extended_levels(oracle, level):
    for index, (name, data, B, P, eof) in enumerate(mw.cases(oracle)):
        file, offsets, stored = mw.expected_case(oracle, index, level)
        assert len(offsets) == -(-len(data) // B) + 1 == len(stored) + 1, name
        if file:
            assert gzip.decompress(file) == data, name
        assert [o for o, _ in mw.members_of(file[:offsets[-1]])] == offsets[:-1], name
