"""Inputs of the best-path decode contract (aptai_ctc_greedy_decode = hostlogic.ctc_bracketed_best_path per row), shared by
tests/test_cpu_host.py (which checks without a GPU that the situations below occur) and tests/test_gpu_ctc_ops.py (which decodes
the batch on the device).  One batch per blank id: 6 rows of 130 frames (three 64-frame rounds, the last partial) over 6 tokens,
row lengths 130, 128, 65, 64, 1, 0; a seeded label path with +6 on its token, plus hand-placed frames:
  row 0  label 3 on frames 60..66 (a run across the 63 | 64 round boundary), tokens 3 and 4 exactly equal on frame 10, silence on
         its last frame 129
  row 1  silence on its first frame and on its last own frame 127
  row 2  blank then silence at the start, label 4 on frames 63..64 (its last own frame repeats across the boundary)
  row 3  all blank          row 4  one frame, the silence          row 5  no frame
Frames at and past a row's length hold a non-blank, non-silence winner: read, they change the answer."""
import functools

import numpy as np

from aptai_amd import hostlogic

B, T, V, LDL, ROWS_PER_B, SIL = 6, 130, 6, 64, 133, 1
LENS = (130, 128, 65, 64, 1, 0)
BLANKS = (0, 2)
PAD_TOKEN = 5


@functools.lru_cache(maxsize=None)
def emissions(blank):
    """fp32 [B][T][V].  Computed once per process; do not modify."""
    rs = np.random.RandomState(7 + blank)
    path = np.empty((B, T), dtype=np.int64)
    tok = blank
    for b in range(B):
        for t in range(T):
            u = rs.rand()
            if u < 0.3:
                tok = blank
            elif u >= 0.6:
                tok = int(rs.randint(V))
            path[b, t] = tok
    path[0, 59], path[0, 60:67], path[0, 67] = 5, 3, blank
    path[0, 9], path[0, 10], path[0, 11] = 5, 3, blank
    path[0, 128], path[0, 129] = 3, SIL
    path[1, 0], path[1, 1], path[1, 126], path[1, 127] = SIL, 4, 4, SIL
    path[2, 0], path[2, 1], path[2, 2] = blank, SIL, 3
    path[2, 62], path[2, 63:65] = blank, 4
    path[3] = blank
    path[4, 0] = SIL
    em = (rs.randn(B, T, V) * 0.5).astype(np.float32)
    np.put_along_axis(em, path[:, :, None], np.take_along_axis(em, path[:, :, None], 2) + 6.0, 2)
    em[0, 10] = -1.0
    em[0, 10, 3:5] = 7.0                                          # two exactly equal maxima: the lower id wins
    for b, n in enumerate(LENS):
        em[b, n:] = -1.0
        em[b, n:, PAD_TOKEN] = 8.0
    em.setflags(write=False)
    return em


def padded(blank):
    """The batch as the kernel reads it, fp32 [B * ROWS_PER_B][LDL]: the columns V.. and the rows T.. hold 1e9, larger than any
    logit, so a read outside the contract wins an argmax."""
    full = np.full((B, ROWS_PER_B, LDL), 1e9, dtype=np.float32)
    full[:, :T, :V] = emissions(blank)
    return full.reshape(B * ROWS_PER_B, LDL)


@functools.lru_cache(maxsize=None)
def oracle(blank, sil, own_lens):
    """Per row (tokens int64, timesteps int32) of hostlogic.ctc_bracketed_best_path, each row over its own length or over all T."""
    em = emissions(blank)
    return [hostlogic.ctc_bracketed_best_path(em[b], LENS[b] if own_lens else T, blank, sil) for b in range(B)]


def assert_situations(blank):
    """What the batch is there for, read off the oracle's output (the inputs are checked, not a device result)."""
    em = emissions(blank)
    plain, framed = oracle(blank, None, True), oracle(blank, SIL, True)

    def at(rows, b):                                             # {timestep: token} of a row
        return dict(zip(rows[b][1].tolist(), rows[b][0].tolist()))
    # a run of one label across the 63 | 64 boundary: one token, at the run's first frame
    assert at(plain, 0)[60] == 3 and not set(range(61, 67)) & set(at(plain, 0))
    assert at(plain, 2)[63] == 4 and 64 not in at(plain, 2) and plain[2][1][-1] == 63
    # silence on the first frame merges with the opening one; on the last own frame, with the closing one
    assert at(plain, 1)[0] == SIL and at(framed, 1)[0] == SIL and 1 not in at(framed, 1)
    for b in (0, 1):
        assert plain[b][0][-1] == SIL and plain[b][1][-1] == LENS[b] - 1
        assert framed[b][0][-1] == SIL and framed[b][1][-1] == LENS[b] and framed[b][0][-2] != SIL
    # blank then silence at the start: both silences are kept
    assert framed[2][0][:2].tolist() == [SIL, SIL] and framed[2][1][:2].tolist() == [0, 2]
    # two exactly equal maxima: the lower id
    assert (em[0, 10] == em[0, 10].max()).nonzero()[0].tolist() == [3, 4] and at(plain, 0)[10] == 3 and at(framed, 0)[11] == 3
    # an all-blank row, a one-frame row of silence, the length-0 row
    assert len(plain[3][0]) == 0 and framed[3][0].tolist() == [SIL, SIL] and framed[3][1].tolist() == [0, LENS[3] + 1]
    assert plain[4][0].tolist() == [SIL] and framed[4][0].tolist() == [SIL] and framed[4][1].tolist() == [0]
    assert len(plain[5][0]) == 0 and framed[5][0].tolist() == [SIL] and framed[5][1].tolist() == [0]
    # the frames past a row's length matter: decoding all T frames gives other rows
    for sil in (None, SIL):
        for b in range(1, B):
            assert not np.array_equal(oracle(blank, sil, False)[b][0], oracle(blank, sil, True)[b][0]), (sil, b)
    # and max_n = 5 cuts rows
    assert sum(len(r[0]) > 5 for r in plain) >= 3
