"""The four list walks of the sweeps and every operand source, on the GPU: 256 particles walk lists this file supplies (sph_selftest_walk), after one
workgroup staged a one-run plan through the product's stage_operands, and report what their pair bodies saw -- the number of calls and an
order-sensitive hash of every operand bit and the rigid flag (32-bit, staged and 16-bit walks), or two sequential float32 sums (the quad walk).
numpy computes the same from the dense lists.  Counts run 0 .. 24 at a pitch of 24 entries + the spare group, mixed inside the first two waves,
all zero in the third and all 24 in the fourth (the 32-bit read-ahead then lands in the spare group); slots past a count hold valid indices of
elements that would change the hash; with RIGID, tagged entries are mixed into the first and the last wave and absent from the others."""
import numpy as np
import pytest

from cfd_taichi_amd import _native as nat

pytestmark = pytest.mark.gpu

NP, ROWS, PITCH = nat.WALK_PARTICLES, nat.WALK_ROWS, nat.WALK_PITCH
N_SRC, N_RIG, RUN = 700, 90, (150, 400)                # source arrays, rigid samples, the staged run (first, count)
TAG = np.uint32(0x80000000)
MUL = np.uint32(0x9E3779B1)
MEM_SOURCES = ["p", "a", "ab", "as", "abc"]
LDS_SOURCES = ["f4", "f4_scaled", "ps", "ps_scaled", "pv", "pv_scaled", "f4s", "f4src_b", "update_p"]
MEM_CASES = [(s, r) for s in MEM_SOURCES for r in (False, True) if not (s == "p" and r)]      # (a list of source "p" never holds a tagged entry)


def _values(rng, shape):
    """non-zero, of both signs, magnitudes spread over 2^-20 .. 2^20: any other order of additions shows in a float32 sum"""
    return (np.ldexp(rng.uniform(0.5, 1.0, shape), rng.integers(-19, 21, shape)) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(20261018)
    d = {k: _values(rng, (N_SRC, 4)) for k in "ABC"}
    d["S"] = _values(rng, N_SRC)
    d["RP"] = _values(rng, (N_RIG, 4))
    counts = np.concatenate([rng.permutation(np.arange(128) % (ROWS + 1)), np.zeros(64, int), np.full(64, ROWS)]).astype(np.int32)
    d["counts"] = counts
    tagged = rng.random((NP, PITCH)) < 0.2
    tagged[64:192] = False                              # waves without a tagged entry: the plain side of the wave-uniform branch
    d["tagged"] = tagged
    d["rigid_idx"] = rng.integers(0, N_RIG, (NP, PITCH)).astype(np.uint32)
    d["mem_idx"] = rng.integers(0, N_SRC, (NP, PITCH)).astype(np.uint32)
    d["lds_idx"] = rng.integers(0, RUN[1], (NP, PITCH)).astype(np.uint32)
    return d


def _lists(d, lds, rigid):
    fluid = d["lds_idx"] if lds else d["mem_idx"]
    return np.where(d["tagged"], d["rigid_idx"] | TAG, fluid).astype(np.uint32) if rigid else fluid


def _operands(d, src, lds, idx):
    """(words of a fluid entry [n, w] as float32, scaled) for source `src` at the entries idx (local indices for an LDS source)"""
    g = idx.astype(np.int64) + (RUN[0] if lds else 0)
    A, B, C, S = d["A"][g], d["B"][g], d["C"][g], d["S"][g]
    zero = np.zeros_like(A)
    scaled = src.endswith("_scaled")
    pos = A[:, :3] * np.float32(2.0 ** 32) if scaled else A[:, :3]
    col = lambda v: v.reshape(-1, 1)
    if src == "p":
        return A, False
    if src in ("a", "f4", "f4_scaled"):
        return np.hstack([pos, col(A[:, 3]), zero]), scaled                                # body(pj, 0, j)
    if src in ("ps", "ps_scaled"):
        return np.hstack([pos, col(S), zero]), scaled
    if src in ("ab", "f4src_b"):
        return np.hstack([A, B]), False
    if src in ("pv", "pv_scaled"):
        z = col(np.zeros(len(A), np.float32))
        return np.hstack([pos, z, B[:, :3], z]), scaled
    if src in ("as", "f4s"):
        return np.hstack([A, col(S)]), False
    if src == "abc":
        return np.hstack([A, B, C]), False
    assert src == "update_p"
    return np.hstack([A, B, C[:, :3], col(np.zeros(len(A), np.float32))]), False


def _expected(d, src, lds, rigid, lists):
    """calls, hash and the two sums per particle, entry by entry in list order"""
    counts = d["counts"]
    h = np.zeros(NP, np.uint32)
    acc = [np.full(NP, 0.001, np.float32), np.zeros(NP, np.float32)]
    for k in range(ROWS):
        active = k < counts
        j = lists[:, k]
        rg = (j & TAG) != 0
        fw, scaled = _operands(d, src, lds, np.where(rg, 0, j))
        rp = d["RP"][np.where(rg, j & ~TAG, 0)]
        rw = np.hstack([rp[:, :3] * np.float32(2.0 ** 32) if scaled else rp[:, :3], rp[:, 3:4]])
        for words, flag, mask in ((fw, 0, active & ~rg), (rw, 1, active & rg)):
            words = np.ascontiguousarray(words, np.float32).view(np.uint32)
            for w in range(words.shape[1]):
                h = np.where(mask, h * MUL + words[:, w], h)
            h = np.where(mask, h * MUL + np.uint32(flag), h)
        first = np.where(rg, rw[:, 0], fw[:, 0]).astype(np.float32), np.where(rg, rw[:, 1], fw[:, 1]).astype(np.float32)
        for n in range(2):
            acc[n] = np.where(active, acc[n] + first[n], acc[n]).astype(np.float32)
    return counts.astype(np.uint32), h, acc


def _run(d, walk, src, rigid):
    lds = walk in ("staged", "list16")
    lists = _lists(d, lds, rigid)
    got = nat.selftest_walk(walk, src, rigid, lists, d["counts"], RUN, d["A"], d["B"], d["C"], d["S"], d["RP"])
    return got, _expected(d, src, lds, rigid, lists)


@pytest.mark.parametrize("src,rigid", MEM_CASES)
def test_walk_list(data, src, rigid):
    got, (calls, h, _) = _run(data, "list", src, rigid)
    assert np.array_equal(got[:, 0], calls)
    assert np.array_equal(got[:, 1], h)


@pytest.mark.parametrize("rigid", [False, True])
@pytest.mark.parametrize("src", LDS_SOURCES)
def test_walk_staged(data, src, rigid):
    got, (calls, h, _) = _run(data, "staged", src, rigid)
    assert np.array_equal(got[:, 0], calls)
    assert np.array_equal(got[:, 1], h)


@pytest.mark.parametrize("src", LDS_SOURCES)
def test_walk_list16(data, src):
    got, (calls, h, _) = _run(data, "list16", src, False)
    assert np.array_equal(got[:, 0], calls)
    assert np.array_equal(got[:, 1], h)


@pytest.mark.parametrize("src,rigid", MEM_CASES)
def test_walk_quad_adds_in_list_order(data, src, rigid):
    got, (_, _, acc) = _run(data, "quad", src, rigid)
    for lane in range(4):                                # the four lanes of a quad hold the same sums
        assert np.array_equal(got[lane::4, 2], acc[0].view(np.uint32))
        assert np.array_equal(got[lane::4, 3], acc[1].view(np.uint32))
