"""What the batches of tests/starts_batches.py hold (CPU, model only), so that
tests/test_gpu_starts.py cannot pass on inputs that exercise nothing."""
import numpy as np

import fide_positions as F
import outcome_model as M
import starts_batches as SB


def test_mixed_batch_holds_every_class():
    b, e = SB.mixed(), SB.mixed_expected()
    assert 200 <= b.n <= 400 and b.moves.shape[0] == SB.N_PLIES
    print(b.n, e.counts, e.stats)
    # both sides to move inside every whole 64-game wave, neighbours with different starts
    stm = np.array([p.stm for p in b.starts])
    for w in range(b.n // 64):
        assert 8 <= int(stm[64 * w:64 * w + 64].sum()) <= 56, w
    seeded = b.n - len(SB.CLOCKS) - 3
    assert all(b.starts[g] is not b.starts[g + 1] for g in range(seeded - 1))
    assert int((stm[:seeded - 1] != stm[1:seeded]).sum()) >= seeded // 4
    # every start clock, and every clock on a game that plays at least one move (150 aside: it is over)
    assert sorted(set(b.clocks.tolist())) == sorted(SB.CLOCKS)
    for hm in SB.CLOCKS:
        played = [g for g in range(b.n) if b.clocks[g] == hm and e.games[g]["accepted"] > 0]
        assert (len(played) == 0) if hm == 150 else (len(played) >= 10), hm
    # starts that are over: mate, stalemate, dead, each at ply 0 with nothing validated
    by_label = {l: g for g, l in enumerate(b.labels)}
    assert e.outcomes[by_label["start_mate"]][:2] == (M.BLACK_WINS, 0)
    assert e.outcomes[by_label["start_stalemate"]][:2] == (M.STALEMATE, 0)
    assert e.outcomes[by_label["start_dead"]][:2] == (M.DEAD, 0)
    # the shuffle: fivefold from 0, 1, 99 and 134 (at 134 the 150th half-move falls on the same ply), the
    # 75-move rule first from 140 and 149, over at ply 0 from 150
    for hm, want in ((0, (M.FIVEFOLD, 16, 5, 16)), (1, (M.FIVEFOLD, 16, 5, 17)), (99, (M.FIVEFOLD, 16, 5, 115)),
                     (134, (M.FIVEFOLD, 16, 5, 150)), (140, (M.SEVENTYFIVE, 10, 3, 150)),
                     (149, (M.SEVENTYFIVE, 1, 1, 150)), (150, (M.SEVENTYFIVE, 0, 1, 150))):
        assert e.outcomes[by_label["shuffle_%d" % hm]] == want, hm
    assert e.counts[M.FIVEFOLD] >= 4 and e.counts[M.SEVENTYFIVE] >= 10 and e.counts[M.ONGOING] >= 100
    assert min(e.counts) >= 1
    # seventy-five in the middle of a seeded game, not only at ply 0 or 1
    assert sum(1 for g in range(seeded) if e.outcomes[g][0] == M.SEVENTYFIVE and e.outcomes[g][1] >= 10) >= 3
    # first moves that need the start's own castle and ep fields, accepted
    ep = castle = 0
    for g, r in enumerate(e.games):
        if r["accept"][0]:
            m, p = int(b.moves[0, g]), b.starts[g]
            f, t = m & 63, (m >> 6) & 63
            kind = int(p.cells[f]) & 7
            ep += kind == F.P and t == p.ep
            castle += kind == F.K and abs(t - f) == 2
    assert ep >= 4 and castle >= 4, (ep, castle)
    # rejected plies, and final positions that differ from the starts and from each other
    assert e.stats["rejected"] >= 1000 and e.stats["accepted"] >= 2000
    moved = ~SB.same_pos(e.finals, b.dstarts).all(axis=1)
    assert int(moved.sum()) >= 150
    assert len({bytes(x) for x in e.finals.view(np.uint8).reshape(b.n, 40)}) >= 150
    assert not e.finals["r0"].any() and not e.finals["r1"].any()


def test_mixed_resolver_tokens():
    b, e, r = SB.mixed(), SB.mixed_expected(), SB.mixed_resolve()
    print(r.counts.tolist())
    tokens, resolved, nomatch, ambiguous, malformed = r.counts.tolist()
    assert tokens == resolved + nomatch + ambiguous + malformed
    assert resolved >= 2000 and nomatch >= 300 and ambiguous >= 1
    assert int((r.first_bad < SB.N_PLIES).sum()) >= 50 and int((r.first_bad == SB.N_PLIES).sum()) >= 50
    # the resolver does not adjudicate: where the replay stops at a clock, it does not, and a
    # repeated token can take a game off the played line -- finals differ between the two
    same = SB.same_pos(r.finals, e.finals).all(axis=1)
    assert int(same.sum()) >= 100 and int((~same).sum()) >= 5


def test_shuffle_wave():
    b = SB.shuffle_wave()
    e = SB.Expected(b)
    assert b.n == 64 and len(set(b.clocks.tolist())) == len(SB.CLOCKS)
    assert {o[0] for o in e.outcomes} == {M.FIVEFOLD, M.SEVENTYFIVE}
    assert len(set(e.outcomes)) == len(SB.CLOCKS)  # every clock ends its own way


def test_distinct_starts():
    b = SB.distinct_starts()
    e = SB.Expected(b)
    assert b.n == 257
    assert len({(p.cells.tobytes(), p.stm, p.castle, p.ep) for p in b.starts}) == 257
    # game 256 is not game 0: another start, another clock or another outcome
    assert not SB.same_pos(b.dstarts[256:], b.dstarts[:1]).all()
    assert e.digests[256] != e.digests[0] and not SB.same_pos(e.finals[256:], e.finals[:1]).all()
    assert len(set(e.digests[:256].tolist()) & set(e.digests[256:].tolist())) == 0
