"""fpldpc_harvest_scan (Harvest.scan_torch) against tests/harvest_model.py, exactly: weight, unsat, err and syn of
random hard words with random garbage in the bits at or above n, for
  * array13x2 (n = 169: 6 words with a partial tail; m = 26 < 64),
  * the irregular code of test_gpu_layered_sat (n = 24 < 32, m = 12, degrees 2..6: -1 padding),
  * array59x2 (degree 59, n = 3481, m = 118 = 64 + 54),
  * A (n = 2209, m = 235 = 7 * 32 + 11),
  * the longest code the loader takes (long_alist(8191): n = 65,528, m = 16,382), batch 3,
with batches 1, 5 and 257 (four frames to a workgroup: a last workgroup with one frame), the sent word NULL,
shared and per frame, err / syn left out, and 0xAA guards behind every buffer.  The ordered compaction of a
chunk (fpldpc_testing_harvest_compact) against numpy at tile edges of its one-workgroup scan."""
import ctypes

import numpy as np
import pytest

import harvest_model as HM
from test_gpu_layered_sat import long_alist, small_code

pytestmark = pytest.mark.gpu
GUARD = 64


@pytest.fixture(scope="module")
def code_of(F):
    made = {}

    def get(which):
        if which not in made:
            code = (F.Code.array(47, 5) if which == "A" else F.Code.parse(long_alist(8191)) if which == "long"
                    else small_code(F, which)[0])
            made[which] = (code, code.lists()[3], F.Harvest(code, 0))
        return made[which]
    return get


def guarded(torch, dev, words, dtype):
    """A tensor of `words` elements followed by GUARD elements of 0xAA bytes; (whole, view of the front)."""
    whole = torch.full((words + GUARD,), -0x55555556 if dtype == torch.int32 else 0xAA, dtype=dtype, device=dev)
    return whole, whole[:words]


def run_case(F, dev, code, clist, hv, batch, cw_mode, patterns, seed):
    import torch
    rng = np.random.default_rng(seed)
    n, m, hw, sw = code.n, code.m, hv.hard_words, hv.syn_words
    words = rng.integers(0, 1 << 32, (batch, hw), dtype=np.uint64).astype(np.uint32)  # garbage above n included
    if n % 32:
        words[:, -1] |= np.uint32(1 << 31)  # whatever the draw
    bits = F.unpack_hard(words, n)
    cw = {None: None, "shared": rng.integers(0, 2, n).astype(np.uint8),
          "frame": rng.integers(0, 2, (batch, n)).astype(np.uint8)}[cw_mode]
    want_w, want_u, e, s = HM.scan(bits, cw, clist)
    hard = torch.from_numpy(words.view(np.int32)).to(dev)
    # bit in the LSB: the other bits of a codeword byte are not read
    cw_t = None if cw is None else torch.from_numpy(cw | (rng.integers(0, 128, cw.shape).astype(np.uint8) << 1)).to(dev)
    bufs = {"weight": guarded(torch, dev, batch, torch.int32), "unsat": guarded(torch, dev, batch, torch.int32)}
    if patterns:
        bufs["err"] = guarded(torch, dev, batch * hw, torch.int32)
        bufs["syn"] = guarded(torch, dev, batch * sw, torch.int32)
    ptr = {k: v[1].data_ptr() for k, v in bufs.items()}
    hv.scan_ptrs(hard.data_ptr(), cw_t.data_ptr() if cw is not None else 0, 1 if cw_mode == "frame" else 0, batch,
                 ptr["weight"], ptr["unsat"], ptr.get("err", 0), ptr.get("syn", 0),
                 torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    got = {k: v[0].cpu().numpy() for k, v in bufs.items()}
    for k, a in got.items():
        assert (a[-GUARD:].view(np.uint8) == 0xAA).all(), f"{k}: written past the end"
    assert (got["weight"][:batch] == want_w).all() and (got["unsat"][:batch] == want_u).all()
    if patterns:
        assert (got["err"][:-GUARD].view(np.uint32).reshape(batch, hw) == HM.pack(e)).all()
        assert (got["syn"][:-GUARD].view(np.uint32).reshape(batch, sw) == HM.pack(s)).all()
    return want_w, want_u


@pytest.mark.parametrize("cw_mode", [None, "shared", "frame"])
@pytest.mark.parametrize("batch", [1, 5, 257])
@pytest.mark.parametrize("which", ["array13x2", "irregular", "array59x2", "A"])
def test_scan_equals_the_model(F, torch_dev, code_of, which, batch, cw_mode):
    code, clist, hv = code_of(which)
    if which == "irregular":
        assert (clist < 0).any() and code.n < 32 and code.m < 64
    w, u = run_case(F, torch_dev, code, clist, hv, batch, cw_mode, True, seed=batch)
    assert w.max() > 0 and u.max() > 0
    run_case(F, torch_dev, code, clist, hv, batch, cw_mode, False, seed=batch)  # err / syn NULL: the rest unchanged


@pytest.mark.parametrize("cw_mode", [None, "shared", "frame"])
def test_longest_code(F, torch_dev, code_of, cw_mode):
    code, clist, hv = code_of("long")
    assert code.n == 65528 and hv.hard_words == 2048 and hv.syn_words == 512
    run_case(F, torch_dev, code, clist, hv, 3, cw_mode, True, seed=9)


def test_codewords_have_weight_and_unsat_zero(F, torch_dev, code_of):
    """Hard decisions equal to the sent codewords, garbage above n: (0, 0) for every frame; one flipped bit in
    frame 3: weight 1 and that variable's checks."""
    import torch
    code, clist, hv = code_of("array13x2")
    enc = F.Encoder.from_code(code)
    cw = enc.encode(np.random.default_rng(1).integers(0, 2, (9, enc.k)).astype(np.uint8))
    words = HM.pack(cw)
    words[:, -1] |= np.uint32(0xFFFFFFFF) << np.uint32(code.n % 32)
    words[3, 2] ^= np.uint32(1 << 5)  # variable 69
    out = hv.scan_torch(torch.from_numpy(words.view(np.int32)).to(torch_dev), torch.from_numpy(cw).to(torch_dev))
    w, u = out["weight"].cpu().numpy(), out["unsat"].cpu().numpy()
    assert w.tolist() == [0, 0, 0, 1, 0, 0, 0, 0, 0] and u.tolist() == [0, 0, 0, code.dv_max, 0, 0, 0, 0, 0]
    syn = F.unpack_hard(out["syn"].cpu().numpy(), code.m)[3]
    assert sorted(np.nonzero(syn)[0]) == sorted(c for c in range(code.m) if 69 in clist[c])
    assert np.nonzero(F.unpack_hard(out["err"].cpu().numpy(), code.n)[3])[0].tolist() == [69]


@pytest.mark.parametrize("batch,cap,every", [(1, 1, 1), (255, 300, 2), (256, 7, 1), (257, 257, 1), (1000, 64, 3),
                                             (1000, 1000, 1), (513, 5, 1000)])
def test_compaction_is_ordered_and_bounded(F, torch_dev, batch, cap, every):
    """Rows of the frames with weight > 0, in frame order, the first `cap` of them; records past the last one
    and the guard behind the buffer untouched.  Tiles of 256 frames: batches at and around the tile size."""
    import torch
    rng = np.random.default_rng(batch + cap)
    row_words = 7
    weight = np.where(np.arange(batch) % every == 0, rng.integers(1, 9, batch), 0).astype(np.int32)
    weight[rng.integers(0, batch)] = 0
    rows = rng.integers(0, 1 << 31, (batch, row_words)).astype(np.int32)
    bad = np.nonzero(weight > 0)[0][:cap]
    rec_whole, rec = guarded(torch, torch_dev, cap * row_words, torch.int32)
    pos = torch.empty(batch, dtype=torch.int32, device=torch_dev)
    c = ctypes.c_void_p
    weight_t, rows_t = torch.from_numpy(weight).to(torch_dev), torch.from_numpy(rows).to(torch_dev)
    st = F.lib().fpldpc_testing_harvest_compact(c(weight_t.data_ptr()), c(rows_t.data_ptr()), row_words, batch, cap,
                                                c(pos.data_ptr()), c(rec.data_ptr()),
                                                c(torch.cuda.current_stream(torch_dev).cuda_stream))
    assert st == 0
    torch.cuda.synchronize()
    got = rec_whole.cpu().numpy()
    want_pos = np.full(batch, -1, np.int32)
    want_pos[bad] = np.arange(len(bad))
    assert (pos.cpu().numpy() == want_pos).all()
    assert (got[:len(bad) * row_words].reshape(-1, row_words) == rows[bad]).all()
    assert (got[len(bad) * row_words:].view(np.uint8) == 0xAA).all()  # nothing else written
