"""tests/harvest_model.py on hand-made cases: a single flipped bit, a whole codeword flipped (weight > 0 with
every check satisfied: an undetected error), the -1 padding of mixed degrees, first-N truncation.  CPU only."""
import numpy as np

import harvest_model as HM

# 3 checks over 7 variables, degrees 4, 3 and 2: the rows of the shorter checks end in -1
CLIST = np.array([[0, 1, 2, 4], [1, 2, 5, -1], [3, 6, -1, -1]])
CODEWORD = np.array([1, 1, 0, 0, 0, 1, 0], np.uint8)  # check 0: 1+1+0+0, check 1: 1+0+1, check 2: 0+0


def test_pack():
    bits = np.zeros((2, 35), np.uint8)
    bits[0, [0, 31, 34]] = 1
    bits[1, 32] = 1
    assert HM.pack(bits).tolist() == [[0x80000001, 0x4], [0, 1]]
    assert HM.pack(np.zeros((0, 35), np.uint8)).shape == (0, 2)


def test_a_codeword_is_clean_and_one_flip_shows_in_its_checks():
    hard = np.tile(CODEWORD, (3, 1))
    hard[1, 2] ^= 1  # variable 2 is in checks 0 and 1
    hard[2, 6] ^= 1  # variable 6 is in check 2 alone
    w, u, e, s = HM.scan(hard, CODEWORD, CLIST)
    assert w.tolist() == [0, 1, 1] and u.tolist() == [0, 2, 1]
    assert s.tolist() == [[0, 0, 0], [1, 1, 0], [0, 0, 1]]
    assert np.nonzero(e[1])[0].tolist() == [2] and np.nonzero(e[2])[0].tolist() == [6]


def test_padding_is_not_variable_zero_or_the_last_one():
    """A -1 slot read as variable 0 would flip checks 1 and 2 with bit 0; read as index -1, with bit 6."""
    hard = np.zeros((2, 7), np.uint8)
    hard[0, 0] = 1
    hard[1, 6] = 1
    _, u, _, s = HM.scan(hard, None, CLIST)
    assert s.tolist() == [[1, 0, 0], [0, 0, 1]] and u.tolist() == [1, 1]


def test_the_syndrome_is_taken_on_the_hard_decision_not_on_the_error():
    """Sent word not a codeword (a shortened or forced frame): hard = sent has weight 0 and unsat > 0."""
    sent = np.array([1, 0, 0, 0, 0, 0, 0], np.uint8)
    w, u, _, _ = HM.scan(sent[None], sent, CLIST)
    assert w.tolist() == [0] and u.tolist() == [1]


def test_whole_codeword_flipped_is_undetected():
    hard = np.stack([CODEWORD, np.zeros(7, np.uint8), CODEWORD ^ np.array([0, 0, 0, 1, 0, 0, 0], np.uint8)])
    h = HM.harvest(hard, CODEWORD, CLIST, iters=[1, 7, 7], blk=[0, 2, 0], first_frame=37)
    assert h["counts"] == dict(frames=3, codeword_errors=2, detected=1, undetected=1, recorded=2, dropped=0)
    assert h["classes"] == {(1, 1): 1, (3, 0): 1} and list(h["classes"]) == [(1, 1), (3, 0)]
    r = h["records"]
    assert r["frame"].tolist() == [38, 39] and r["iters"].tolist() == [7, 7] and r["info_errors"].tolist() == [2, 0]
    assert r["weight"].tolist() == [3, 1] and r["unsat"].tolist() == [0, 1]
    assert r["err"].tolist() == [[0b0100011], [0b0001000]] and r["syn"].tolist() == [[0], [0b100]]
    assert r["frame"].dtype == np.int64 and r["err"].dtype == np.uint32 and r["weight"].dtype == np.int32


def test_per_frame_codewords_and_first_n():
    rng = np.random.default_rng(3)
    cw = rng.integers(0, 2, (40, 7)).astype(np.uint8)
    hard = cw.copy()
    flips = [3, 4, 9, 20, 39]
    for f in flips:
        hard[f, f % 7] ^= 1
    its, blk = np.arange(40), np.arange(40) % 3
    full = HM.harvest(hard, cw, CLIST, its, blk)
    assert full["records"]["frame"].tolist() == flips and full["counts"]["codeword_errors"] == 5
    assert (full["records"]["weight"] == 1).all()
    cut = HM.harvest(hard, cw, CLIST, its, blk, max_records=2)
    assert cut["counts"] == {**full["counts"], "recorded": 2, "dropped": 3} and cut["classes"] == full["classes"]
    for k in HM.FIELDS:
        assert (cut["records"][k] == full["records"][k][:2]).all()
    none = HM.harvest(hard, cw, CLIST, its, blk, max_records=0)
    assert none["counts"]["recorded"] == 0 and none["records"]["err"].shape == (0, 1) and none["classes"] == full["classes"]
