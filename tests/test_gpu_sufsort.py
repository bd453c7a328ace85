"""GPU: the sufsort module (amd.set_suffix_sort, amd.set_bwt, amd.suffix_sort, amd.bwt) against the brute-force restatement of
tests/test_sufsort_oracle.py: suffixes, global indices, BWT bytes and the count equal bit for bit, with and without
SUFSORT_NO_EMPTY_SUFFIXES; the work the sorter reports stays proportional to the ties; a 20 M-suffix read set is proved sorted
without brute force; the single-string entries equal the oracle's suffix array and the index build's BWT."""
import numpy as np
import pytest

import test_sufsort_oracle as S
from test_gpu_qgram import _string_set, pack, text_of

pytestmark = pytest.mark.gpu

W = {2: 29, 4: 15, 8: 7}                                             # symbols per key word (nvbio_sufsort_stats::symbols_per_word)


def max_rounds(strings, bits):
    max_len = max([len(s) for s in strings], default=0)
    return -(-(max_len + 1) // W[bits])


def check_set(amd, sset, strings, bits):
    """both calls, both flag values, against the brute force; -> the stats of the plain sort"""
    out = None
    for flags in (0, amd.SUFSORT_NO_EMPTY_SUFFIXES):
        want_suf, want_glb, want_bwt = S.set_suffix_sort(strings, no_empty=bool(flags))
        n = amd.set_suffix_count(sset, flags)
        assert n == len(want_glb) == sum(len(s) + (0 if flags else 1) for s in strings)
        suf, glb, st = amd.set_suffix_sort(sset, flags)
        assert np.array_equal(amd.u32(suf).reshape(-1, 2), want_suf)
        assert np.array_equal(amd.u32(glb), want_glb)
        bwt, suf2, st2 = amd.set_bwt(sset, flags)
        assert np.array_equal(bwt.cpu().numpy(), want_bwt)
        assert np.array_equal(amd.u32(suf2).reshape(-1, 2), want_suf)
        sa, ids, cum, st3 = amd.set_suffix_sort_flat(sset, flags)                  # the reference's handler form
        assert np.array_equal(amd.u32(sa), want_glb) and np.array_equal(amd.u32(ids), want_suf[:, 1])
        assert np.array_equal(amd.u32(cum), np.cumsum([len(s) + (0 if flags else 1) for s in strings]).astype(np.uint32))
        assert st3["sorted_per_round"] == st["sorted_per_round"]
        only_bwt, none, _ = amd.set_bwt(sset, flags, want_suffixes=False)
        assert none is None and np.array_equal(only_bwt.cpu().numpy(), want_bwt)
        for s in (st, st2):
            assert s["n_suffixes"] == n and s["symbols_per_word"] == W[bits]
            assert s["rounds"] <= max_rounds(strings, bits), (s, max_rounds(strings, bits))
            assert s["sorted_per_round"][0] == n and (n == 0) == (s["rounds"] == 0)
            assert all(a >= b for a, b in zip(s["sorted_per_round"], s["sorted_per_round"][1:]))
        assert st["sorted_per_round"] == st2["sorted_per_round"]
        if out is None:
            out = st
    return out


def ragged_set(amd, orc, strings, bits, lead=0):
    syms = np.concatenate([np.full(lead, 3, np.uint8)] + [np.asarray(s, np.uint8) for s in strings])
    offs = np.zeros(len(strings) + 1, np.uint32)
    offs[1:] = np.cumsum([len(s) for s in strings])
    return amd.PackedStringSet(pack(orc, syms, bits), bits, len(strings), offsets=offs + lead, ranges=True)


@pytest.mark.parametrize("layout", ["fixed", "ragged", "offset"])
@pytest.mark.parametrize("bits", [2, 4, 8])
def test_random_sets(amd, orc, layout, bits):
    rng = np.random.default_rng(bits * 7 + len(layout))
    lens = [150] * 40 if layout == "fixed" else list(rng.integers(0, 80, 60)) + [3, 4, 5, 19, 20, 21]
    strings = [text_of(rng, int(L), bits, with_n=True) for L in lens]
    if bits == 8:
        strings[1][:] = rng.integers(0, 256, len(strings[1]))        # every byte value sorts by its raw value
    check_set(amd, _string_set(amd, orc, strings, bits, layout), strings, bits)


def test_fixed_length_starts_without_ranges(amd, orc):
    """n start offsets plus fixed_len: strings that overlap and are out of order in the symbol stream"""
    rng = np.random.default_rng(3)
    text = text_of(rng, 4000, 2)
    starts = rng.integers(0, 4000 - 70, 50).astype(np.uint32)
    strings = [text[s:s + 70] for s in starts]
    sset = amd.PackedStringSet(orc.pack2(text), 2, len(strings), offsets=starts, fixed_len=70)
    check_set(amd, sset, strings, 2)


@pytest.mark.parametrize("bits", [2, 4, 8])
def test_fixed_stride_with_padding_between_strings(amd, orc, bits):
    """stride != fixed_len: 30 symbols of every 41 are a string, the 11 between are other symbols that must not be read as part of it"""
    rng = np.random.default_rng(40 + bits)
    n, L, stride = 60, 30, 41
    stream = text_of(rng, n * stride, bits, with_n=True)
    strings = [stream[i * stride:i * stride + L].copy() for i in range(n)]
    strings[7] = strings[3].copy()
    stream[7 * stride:7 * stride + L] = strings[3]                    # equal strings whose paddings differ
    stream[7 * stride + L:8 * stride] = 3
    sset = amd.PackedStringSet(pack(orc, stream, bits), bits, n, fixed_len=L, stride=stride)
    check_set(amd, sset, strings, bits)


@pytest.mark.parametrize("layout", ["fixed", "ragged"])
def test_four_bit_symbols_up_to_15(amd, orc, layout):
    """every 4-bit value, the top bit of the symbol (and of the 64-bit key word) included"""
    rng = np.random.default_rng(15)
    lens = [47] * 50 if layout == "fixed" else list(rng.integers(0, 70, 70))
    strings = [rng.integers(0, 16, int(L), dtype=np.uint8) for L in lens]
    run = 47                                                          # three full words and a part
    strings += [np.full(run, 15, np.uint8), np.full(run, 15, np.uint8), np.full(run, 8, np.uint8)]
    st = check_set(amd, _string_set(amd, orc, strings, 4, layout), strings, 4)
    assert st["rounds"] >= 2                                          # the runs of 15 tie past the first word


def sample_reads(rng, genome_len, n_reads, read_len):
    genome = rng.integers(0, 4, genome_len, dtype=np.uint8)
    starts = rng.integers(0, genome_len - read_len + 1, n_reads)
    return genome, starts


def test_reads_with_deep_ties_across_strings(amd, orc):
    """2,000 reads of 100 bp at 40x from a 5 kbp genome: nearly every suffix ties with the overlapping reads' for several words"""
    rng = np.random.default_rng(11)
    genome, starts = sample_reads(rng, 5000, 2000, 100)
    strings = [genome[s:s + 100] for s in starts]
    st = check_set(amd, amd.PackedStringSet(orc.pack2(np.concatenate(strings)), 2, 2000, fixed_len=100), strings, 2)
    assert st["rounds"] == 4 and st["sorted_per_round"][1] > st["n_suffixes"] // 2
    check_set(amd, ragged_set(amd, orc, strings, 4), strings, 4)


def test_all_a_ragged(amd, orc):
    strings = [np.zeros(L, np.uint8) for L in range(201)]
    for bits in (2, 8):
        check_set(amd, ragged_set(amd, orc, strings[::-1] + strings, bits), strings[::-1] + strings, bits)


def test_copies_of_one_string(amd, orc):
    rng = np.random.default_rng(5)
    strings = [text_of(rng, 77, 2)] * 500
    check_set(amd, amd.PackedStringSet(orc.pack2(np.concatenate(strings)), 2, 500, fixed_len=77), strings, 2)


@pytest.mark.parametrize("bits", [2, 4, 8])
def test_lengths_around_the_word(amd, orc, bits):
    rng = np.random.default_rng(bits)
    w = W[bits]
    base = text_of(rng, 2 * w + 2, bits)
    strings = []
    for L in (w - 1, w, w + 1, 2 * w - 1, 2 * w, 2 * w + 1):
        strings += [base[:L].copy(), base[:L].copy(), np.zeros(L, np.uint8), text_of(rng, L, bits)]
    check_set(amd, ragged_set(amd, orc, strings, bits, lead=5), strings, bits)


def test_empty_strings_and_empty_set(amd, orc):
    rng = np.random.default_rng(9)
    e = np.zeros(0, np.uint8)
    strings = [e, e, text_of(rng, 40, 4), e, text_of(rng, 33, 4), e, e, text_of(rng, 1, 4), e]
    check_set(amd, ragged_set(amd, orc, strings, 4), strings, 4)
    check_set(amd, ragged_set(amd, orc, [e, e, e], 2), [e, e, e], 2)
    st = check_set(amd, amd.PackedStringSet(np.zeros(16, np.uint8), 8, 0, offsets=np.zeros(1, np.uint32), ranges=True), [], 8)
    assert st["rounds"] == 0 and st["n_suffixes"] == 0
    check_set(amd, amd.PackedStringSet(np.zeros(16, np.uint32), 2, 0, fixed_len=100), [], 2)


def test_four_bit_set_with_n(amd, orc):
    rng = np.random.default_rng(13)
    strings = [text_of(rng, 60, 4) for _ in range(50)]
    for s in strings[::3]:
        s[rng.integers(0, 60, 4)] = 4                                 # N
    strings += [np.full(45, 4, np.uint8), np.full(46, 4, np.uint8)]
    st = check_set(amd, ragged_set(amd, orc, strings, 4), strings, 4)
    assert st["rounds"] == 4                                           # the runs of N tie through every word


def test_two_calls_give_equal_bytes(amd, orc):
    rng = np.random.default_rng(17)
    genome, starts = sample_reads(rng, 3000, 1500, 80)
    sset = amd.PackedStringSet(orc.pack2(np.concatenate([genome[s:s + 80] for s in starts])), 2, 1500, fixed_len=80)
    a = amd.set_suffix_sort(sset)
    b = amd.set_suffix_sort(sset)
    assert np.array_equal(amd.u32(a[0]), amd.u32(b[0])) and np.array_equal(amd.u32(a[1]), amd.u32(b[1])) and a[2] == b[2]
    assert np.array_equal(amd.set_bwt(sset)[0].cpu().numpy(), amd.set_bwt(sset)[0].cpu().numpy())


def test_limits_and_capacity(amd, orc):
    rng = np.random.default_rng(19)
    strings = [text_of(rng, 30, 2) for _ in range(10)]
    words = orc.pack2(np.concatenate(strings))
    good = amd.PackedStringSet(words, 2, 10, fixed_len=30)
    n = amd.set_suffix_count(good)
    assert n == 310 and amd.set_suffix_count(good, amd.SUFSORT_NO_EMPTY_SUFFIXES) == 300

    def invalid(call, *a, **kw):
        with pytest.raises(amd.NvbioError) as e:
            call(*a, **kw)
        assert e.value.status == 1, e.value
        return str(e.value)

    for call in (amd.set_suffix_sort, amd.set_bwt, amd.set_suffix_count):
        for bits in (1, 3, 16):
            bad = amd.PackedStringSet(words, 2, 10, fixed_len=30)
            bad.bits = bits
            assert "symbol_bits" in invalid(call, bad)
        assert "seed" in invalid(call, amd.PackedStringSet(words, 2, 10, fixed_len=10, stride=30, seeds_per_string=2, seed_interval=5))
        assert "flag" in invalid(call, good, 2)
        # sum( len + 1 ) must stay below 2^32 - 1, with or without the flag; nothing reads the symbols of a set that large
        big = amd.PackedStringSet(words, 2, 1 << 20, fixed_len=4095)
        for flags in (0, amd.SUFSORT_NO_EMPTY_SUFFIXES):
            assert "2^32 - 1" in invalid(call, big, flags)
    assert amd.set_suffix_count(amd.PackedStringSet(words, 2, 1 << 20, fixed_len=4094)) == (1 << 20) * 4095
    for call in (amd.set_suffix_sort, amd.set_bwt):
        msg = invalid(call, good, 0, True, n - 1)
        assert "capacity 309" in msg and "310" in msg
        assert len(call(good, 0, True, n + 5)[0]) == n                    # a larger capacity is fine


@pytest.fixture(scope="module")
def random_2bit_200k(amd):
    import torch
    g = torch.Generator(device="cuda:0").manual_seed(23)
    syms = torch.randint(0, 4, (200_000, 100), dtype=torch.uint8, device="cuda:0", generator=g)
    return syms, packed2(amd, syms)


def packed2(amd, syms):
    """a [N, L] uint8 symbol tensor as a fixed-stride 2-bit set (packed on the GPU: big-endian words of 16 symbols)"""
    import torch
    flat = syms.reshape(-1).to(torch.int64)
    pad = (-flat.numel()) % 16
    flat = torch.cat([flat, torch.zeros(pad + 64, dtype=torch.int64, device=flat.device)]).reshape(-1, 16)
    words = (flat << (30 - 2 * torch.arange(16, device=flat.device))).sum(dim=1)
    words = torch.where(words >= (1 << 31), words - (1 << 32), words).to(torch.int32)
    return amd.PackedStringSet(words, 2, syms.shape[0], fixed_len=syms.shape[1])


def test_work_stays_proportional_on_random_reads(amd, random_2bit_200k):
    """200,000 random 100 bp reads: identical full-word keys are expected n^2 / 2 / 4^29 << 1 times, so round 1 sees next to nothing"""
    _, sset = random_2bit_200k
    suf, glb, st = amd.set_suffix_sort(sset)
    n = st["n_suffixes"]
    assert n == 200_000 * 101
    assert st["sorted_per_round"][1] < n // 100, st
    assert st["rounds"] <= -(-101 // 29)


def assert_sorted(torch, syms, suf, chunk=1 << 18):
    """every adjacent pair of the sorted suffixes (pos, string_id) of the [N, L] set ordered: by symbols with the end below every
    symbol, then by string id"""
    N, L = syms.shape
    padded = torch.cat([syms.to(torch.int16), torch.full((N, L + 1), -1, dtype=torch.int16, device=syms.device)], dim=1).reshape(-1)
    cols = torch.arange(L + 1, device=syms.device)
    pos, sid = suf[:, 0].to(torch.int64), suf[:, 1].to(torch.int64)
    for b in range(0, suf.shape[0] - 1, chunk):
        e = min(b + chunk, suf.shape[0] - 1)
        a = padded[((sid[b:e] * (2 * L + 1) + pos[b:e])[:, None] + cols)]
        c = padded[((sid[b + 1:e + 1] * (2 * L + 1) + pos[b + 1:e + 1])[:, None] + cols)]
        diff = a != c
        first = torch.argmax(diff.to(torch.uint8), dim=1)
        same = ~diff.any(dim=1)
        av = torch.gather(a, 1, first[:, None])[:, 0]
        cv = torch.gather(c, 1, first[:, None])[:, 0]
        ok = torch.where(same, sid[b:e] < sid[b + 1:e + 1], av < cv)
        assert bool(ok.all()), "pair %d out of order" % (b + int(torch.nonzero(~ok)[0]))


def test_medium_read_set_is_sorted_and_its_bwt_spells_the_reads(amd):
    """200,000 reads of 100 bp at 30x from a seeded genome, 20.2 M suffixes: the global indices are a permutation and every
    adjacent pair is ordered, which together prove sortedness; and the LF walk from row i spells string i backwards onto a 255"""
    import torch
    dev = "cuda:0"
    N, L = 200_000, 100
    g = torch.Generator(device=dev).manual_seed(29)
    genome = torch.randint(0, 4, (N * L // 30,), dtype=torch.uint8, device=dev, generator=g)
    starts = torch.randint(0, genome.numel() - L + 1, (N,), device=dev, generator=g)
    syms = genome[starts[:, None] + torch.arange(L, device=dev)]
    sset = packed2(amd, syms)
    bwt, suf, st = amd.set_bwt(sset)
    suf2, glb, st2 = amd.set_suffix_sort(sset)
    n = N * (L + 1)
    assert st["n_suffixes"] == n and st["rounds"] <= 4 and st["sorted_per_round"] == st2["sorted_per_round"]
    assert torch.equal(suf, suf2)
    gl = glb.to(torch.int64)
    assert torch.equal(torch.sort(gl).values, torch.arange(n, device=dev))
    assert torch.equal(gl, suf[:, 1].to(torch.int64) * (L + 1) + suf[:, 0].to(torch.int64))
    assert_sorted(torch, syms, suf)
    pos, sid = suf[:, 0].to(torch.int64), suf[:, 1].to(torch.int64)
    want_bwt = torch.where(pos > 0, syms.reshape(-1)[sid * L + torch.clamp(pos - 1, min=0)], torch.full_like(pos, 255).to(torch.uint8))
    assert torch.equal(bwt, want_bwt)

    # LF: C[c] = N + #symbols < c; next = C[c] + #c in bwt[0, row)
    occ = [torch.cumsum((bwt == c).to(torch.int32), 0) - (bwt == c).to(torch.int32) for c in range(4)]    # exclusive counts
    total = torch.tensor([int((bwt == c).sum()) for c in range(4)])
    C = N + torch.cumsum(total, 0) - total
    ids = torch.randperm(N, device=dev, generator=g)[:1000]
    row = ids.clone()
    for step in range(L):
        c = bwt[row].to(torch.int64)
        assert torch.equal(c, syms[ids, L - 1 - step].to(torch.int64)), step
        nxt = torch.zeros_like(row)
        for k in range(4):
            nxt = torch.where(c == k, int(C[k]) + occ[k][row].to(torch.int64), nxt)
        row = nxt
    assert bool((bwt[row] == 255).all())
    assert torch.equal(suf[row][:, 1].to(torch.int64), ids) and bool((suf[row][:, 0] == 0).all())


def _golden_text(fm_golden):
    return np.asarray(fm_golden["text"], np.uint8)


@pytest.mark.parametrize("which", ["golden", "random-1M"])
def test_single_string_entries(amd, orc, fm_golden, which):
    text = _golden_text(fm_golden) if which == "golden" else np.random.default_rng(31).integers(0, 4, 1_000_000, dtype=np.uint8)
    n = len(text)
    words = orc.pack2(text)
    sa = amd.u32(amd.suffix_sort(words, n))
    want = orc.suffix_sort(text)
    assert sa[0] == n and np.array_equal(sa, want)
    if which == "golden":
        assert np.array_equal(sa, S.suffix_array(text)) and np.array_equal(sa[1:], fm_golden["sa"][1:])
    bwt, primary = amd.bwt(words, n)
    fmi = amd.FMIndex.build(words, n)
    bwt_occ, _ = fmi.arrays()
    want_words = amd.u32(bwt_occ).reshape(-1, 8)[:, :4].reshape(-1)[:(n + 15) // 16]
    assert primary == fmi.primary and np.array_equal(amd.u32(bwt), want_words)
    assert primary == int(np.nonzero(sa == 0)[0][0])                  # find_primary
    if which == "golden":
        assert primary == int(fm_golden["primary"])
    fmi.close()


def test_single_string_repeats(amd, orc):
    """a plain suffix sort is not held to the index build's default repeat guard of 4096 symbols; past 2^20 it says so"""
    rng = np.random.default_rng(37)
    text = rng.integers(0, 4, 60_000, dtype=np.uint8)
    text[10_000:15_000] = 0                                           # 5,000 A's
    text[30_000:38_000] = text[40_000:48_000]                         # an 8,000-symbol repeat
    words = orc.pack2(text)
    assert np.array_equal(amd.u32(amd.suffix_sort(words, len(text))), orc.suffix_sort(text))
    bwt, primary = amd.bwt(words, len(text))
    hidx = orc.build_index(text)
    assert primary == hidx.primary
    assert np.array_equal(amd.u32(bwt), hidx.bwt_occ.reshape(-1, 8)[:, :4].reshape(-1)[:(len(text) + 15) // 16])
    n = (1 << 21) + 1000                                              # all A: a repeat longer than 2^20
    zeros = np.zeros(n // 16 + 8, np.uint32)
    for call in (amd.suffix_sort, amd.bwt):
        with pytest.raises(amd.NvbioError) as e:
            call(zeros, n)
        assert e.value.status == 4, e.value                           # NVBIO_ERR_UNSUPPORTED
