"""The case list of tests/test_gpu_code_lengths.py against the oracle alone (no GPU): the guards that keep the device comparison from
passing on histograms that ask nothing of it, the properties any result must have, and zzo_generate on the limiter's lengths."""
from code_length_checks import (ALPHABETS, ANCHORS, CodeOracle, analyse, anchor_input, blocks_over_the_code_length_limit,
                                check_guards, check_lengths)


def rfc1951_codes(lens):
    """RFC 1951 3.2.2, most significant bit first"""
    count = [0] * 17
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, c = [0] * 17, 0
    for b in range(1, 16):
        c = (c + count[b - 1]) << 1
        nxt[b] = c
    out = []
    for l in lens:
        out.append(None if l == 0 else format(nxt[l], "0%db" % l))
        nxt[l] += l != 0
    return out


def test_case_list_guards_hold(oracle):
    A = analyse(oracle)
    check_guards(A)
    for n in ALPHABETS:
        for r in A[n]:
            check_lengths(r, r["want"][0], 0)
            check_lengths(r, r["want"][1], 1, r["want"][0])
            if r["depth"] <= r["maxlen"]:                    # the limit does not bite: package-merge costs what Huffman costs
                assert sum(x * l for x, l in zip(r["f"], r["want"][1])) == sum(x * l for x, l in zip(r["f"], r["want"][0])), r["name"]


def test_generated_codes_are_canonical_and_prefix_free(oracle):
    A = analyse(oracle)
    co = A["co"]
    for n in ALPHABETS:
        for r in A[n]:
            lens = r["want"][0]
            packed = co.generate(lens)
            want = rfc1951_codes(lens)
            words = []
            for l, p, w in zip(lens, packed, want):
                if l == 0:
                    assert p == 0
                    continue
                assert p >> 16 == l
                msb_first = format(p & 0xFFFF, "0%db" % l)[::-1]          # stored bit-reversed (huffman.h:49-81)
                assert msb_first == w, r["name"]
                words.append(msb_first)
            words.sort()
            assert all(not b.startswith(a) for a, b in zip(words, words[1:])), r["name"]


def test_anchor_inputs_cross_the_code_length_limit(oracle):
    """what the end-to-end anchor of the GPU suite rests on: in the oracle's level-2 streams of these inputs, blocks whose code-length
    histogram wants a tree deeper than 7"""
    co = CodeOracle(oracle)
    for name, P in ANCHORS:
        over, blocks = blocks_over_the_code_length_limit(co, oracle.encode_packets(anchor_input(name), 2, 2, P))
        assert over >= 1 and blocks >= 5, (name, over, blocks)
