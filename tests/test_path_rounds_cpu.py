"""The request planner of the path kernels (csrc/path_rounds.hpp): requests of the marginals and of the loop-closure gate -> rounds of
device records.  tests/path_rounds_check.cpp includes the header alone and prints the rounds of a case; the expected rounds are derived
here from the definition -- the path of a column is the column and its ancestors, the common suffix is what two paths share, a request
goes to scratch iff fixed + ylen * 308 + 16 > budget, a round takes its first request and goes on while both caps are not reached --
with hand-written values for the records that matter."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = 308                       # bytes of one path entry: 36 doubles of Y, an int4 record, an int y offset
MARG = dict(width=8, fixed=288, no_column=0, fold=1)
GATE = dict(width=12, fixed=2368, no_column=1, fold=0)
BIG = 1 << 40

# A forest of 12 columns, two components.  Component A: the chain 0-1-2-4-6-7-8 (depth 7) with the branches 3-4 and 5-6; component B:
# 9 and 10 under 11.  Columns 0..5, 9, 10 are poses (6 unknowns), the others landmarks (3).
PARENT = np.array([1, 2, 4, 4, 6, 6, 7, 8, -1, 11, 11, -1])
DIM = np.array([6, 6, 6, 6, 6, 6, 3, 3, 3, 6, 6, 3])
XOFF = np.concatenate([[0], np.cumsum(DIM)[:-1]])
XOFF_COL = np.full(int(DIM.sum()), -1)
XOFF_COL[XOFF] = np.arange(12)


def path(col):
    out = []
    while col >= 0:
        out.append(int(col))
        col = PARENT[col]
    return out


def marg(cu, cv):
    return [int(XOFF[cu]), int(DIM[cu]), int(XOFF[cv]), int(DIM[cv])]


def gate(cu, cv, tag):
    """a gate request; an end None has no column.  The payload is four ints the planner must carry through"""
    end = lambda c: [-1, 6] if c is None else [int(XOFF[c]), int(DIM[c])]
    return end(cu) + end(cv) + [tag, tag + 100, tag + 200, tag % 2]


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    d = tmp_path_factory.mktemp("path_rounds")
    exe = str(d / "path_rounds_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "tests", "path_rounds_check.cpp"), "-o", exe])
    count = [0]

    def run(rules, reqs, budget=60 * 1024, path_cap=BIG, scratch_cap=BIG):
        count[0] += 1
        case = d / f"case{count[0]}.txt"
        words = [len(XOFF_COL), *XOFF_COL, len(PARENT), *PARENT, rules["width"], rules["fixed"], budget, rules["no_column"], rules["fold"],
                 path_cap, scratch_cap, len(reqs), *[v for r in reqs for v in r]]
        case.write_text(" ".join(str(int(w)) for w in words) + "\n")
        out = subprocess.run([exe, str(case)], capture_output=True, text=True)
        assert out.returncode == 0, out.stdout + out.stderr
        lines = out.stdout.split("\n")
        if lines[0] == "refused":
            return None
        rounds = []
        for i in range(0, len(lines) - 1, 3):
            head, up, src = lines[i].split(), lines[i + 1].split(), lines[i + 2].split()
            assert head[0] == "round" and up[0] == "up" and src[0] == "src"
            m, n_lds, ylen_lds, scr = (int(v) for v in head[1:])
            W = rules["width"]
            ints = np.array(up[1:], dtype=np.int64)
            rounds.append(dict(m=m, n_lds=n_lds, ylen_lds=ylen_lds, scr_bytes=scr, recs=ints[:m * W].reshape(m, W), cols=ints[m * W:],
                               src=np.array(src[1:], dtype=np.int64)))
        return rounds
    return run


def expected(rules, reqs, budget=60 * 1024, path_cap=BIG, scratch_cap=BIG):
    """the rounds from the definition"""
    W = rules["width"]
    rounds, k = [], 0
    while k < len(reqs):
        cols, recs, scratch, scr_bytes, k0 = [], [], [], 0, k
        while k < len(reqs) and (k == k0 or (len(cols) < path_cap and scr_bytes < scratch_cap)):
            xu, du, xv, dv = reqs[k][:4]
            pu = path(XOFF_COL[xu]) if xu >= 0 else []
            if rules["fold"] and xu == xv:
                rec = [len(cols), len(pu), len(cols), 0, du, du, len(pu)]
                cols += pu
            else:
                pv = path(XOFF_COL[xv]) if xv >= 0 else []
                shared = set(pu) & set(pv)          # in a forest: the common suffix of the two paths
                rec = [len(cols), len(pu), len(cols) + len(pu), len(pv), du, dv, len(shared)]
                cols += pu + pv
            ylen = rec[1] + rec[3]
            to_scratch = rules["fixed"] + ylen * ENTRY + 16 > budget
            rec.append(scr_bytes // 16 if to_scratch else 0)
            if to_scratch:
                scr_bytes += -(-ylen * ENTRY // 16) * 16
            recs.append(rec + list(reqs[k][4:]))
            scratch.append(to_scratch)
            k += 1
        order = [i for i, s in enumerate(scratch) if not s] + [i for i, s in enumerate(scratch) if s]
        lds = [recs[i] for i in order if not scratch[i]]
        rounds.append(dict(m=len(recs), n_lds=len(lds), ylen_lds=max([r[1] + r[3] for r in lds], default=0), scr_bytes=scr_bytes,
                           recs=np.array([recs[i] for i in order], dtype=np.int64).reshape(len(recs), W), cols=np.array(cols, dtype=np.int64),
                           src=np.array([k0 + i for i in order], dtype=np.int64)))
    return rounds


def same(got, want):
    assert got is not None and len(got) == len(want)
    for g, w in zip(got, want):
        assert (g["m"], g["n_lds"], g["ylen_lds"], g["scr_bytes"]) == (w["m"], w["n_lds"], w["ylen_lds"], w["scr_bytes"])
        for key in ("recs", "cols", "src"):
            assert np.array_equal(g[key], w[key]), key


def rec_paths(rnd, i):
    r = rnd["recs"][i]
    return list(rnd["cols"][r[0]:r[0] + r[1]]), list(rnd["cols"][r[2]:r[2] + r[3]])


def test_marginal_records(planner):
    reqs = [marg(0, 0), marg(3, 0), marg(5, 9), marg(11, 11), marg(10, 9)]
    got = planner(MARG, reqs)
    same(got, expected(MARG, reqs))
    (r,) = got
    assert r["m"] == 5 and r["n_lds"] == 5 and r["scr_bytes"] == 0 and list(r["src"]) == [0, 1, 2, 3, 4]
    # u == v: one path, the second of length 0 at the same place, both dimensions d(u), nc the whole path
    assert list(r["recs"][0]) == [0, 7, 0, 0, 6, 6, 7, 0] and rec_paths(r, 0) == ([0, 1, 2, 4, 6, 7, 8], [])
    # 3 and 0 meet at column 4: the suffix 4-6-7-8
    assert list(r["recs"][1]) == [7, 5, 12, 7, 6, 6, 4, 0] and rec_paths(r, 1) == ([3, 4, 6, 7, 8], [0, 1, 2, 4, 6, 7, 8])
    # different components: nothing shared
    assert list(r["recs"][2]) == [19, 4, 23, 2, 6, 6, 0, 0] and rec_paths(r, 2) == ([5, 6, 7, 8], [9, 11])
    assert list(r["recs"][3]) == [25, 1, 25, 0, 3, 3, 1, 0]
    assert list(r["recs"][4]) == [26, 2, 28, 2, 6, 6, 1, 0]
    assert r["ylen_lds"] == 12


def test_gate_records_and_ends_without_a_column(planner):
    reqs = [gate(3, 0, 10), gate(None, 2, 11), gate(1, None, 12), gate(None, None, 13), gate(9, 5, 14)]
    got = planner(GATE, reqs)
    same(got, expected(GATE, reqs))
    (r,) = got
    assert list(r["recs"][0]) == [0, 5, 5, 7, 6, 6, 4, 0, 10, 110, 210, 0]
    assert list(r["recs"][1]) == [12, 0, 12, 5, 6, 6, 0, 0, 11, 111, 211, 1] and rec_paths(r, 1) == ([], [2, 4, 6, 7, 8])
    assert list(r["recs"][2]) == [17, 6, 23, 0, 6, 6, 0, 0, 12, 112, 212, 0]
    assert list(r["recs"][3]) == [23, 0, 23, 0, 6, 6, 0, 0, 13, 113, 213, 1]
    assert list(r["recs"][4][:8]) == [23, 2, 25, 4, 6, 6, 0, 0]
    assert len(r["cols"]) == 29


def test_marginals_refuse_what_has_no_column(planner):
    assert planner(MARG, [marg(0, 0), [-1, 6, 0, 6]]) is None
    assert planner(MARG, [[0, 6, -1, 6]]) is None
    assert planner(MARG, [[1, 6, 0, 6]]) is None                    # not the start of a block row
    assert planner(MARG, [[0, 6, len(XOFF_COL), 6]]) is None        # past the unknowns
    assert planner(GATE, [[1, 6, -1, 6, 0, 0, 0, 0]]) is None       # the gate forgives a missing column, not a wrong one
    assert planner(GATE, [gate(None, 0, 1)]) is not None


@pytest.mark.parametrize("rules,req,ylen", [(MARG, marg(3, 0), 12), (MARG, marg(0, 0), 7), (GATE, gate(3, 0, 1), 12), (GATE, gate(None, None, 1), 0)])
def test_placement_threshold(planner, rules, req, ylen):
    edge = rules["fixed"] + ylen * ENTRY + 16
    (at,) = planner(rules, [req], budget=edge)
    assert at["n_lds"] == 1 and at["scr_bytes"] == 0 and at["ylen_lds"] == ylen and at["recs"][0][7] == 0
    (below,) = planner(rules, [req], budget=edge - 1)
    assert below["n_lds"] == 0 and below["ylen_lds"] == 0 and below["scr_bytes"] == -(-ylen * ENTRY // 16) * 16
    same([at], expected(rules, [req], budget=edge))
    same([below], expected(rules, [req], budget=edge - 1))


def test_mixed_round_lds_first_in_request_order(planner):
    # paths of 12, 1, 7, 2, 14 and 3 entries; the budget holds 4
    reqs = [marg(3, 0), marg(8, 8), marg(0, 0), marg(7, 7), marg(0, 0 + 1), marg(6, 6)]
    budget = 288 + 4 * ENTRY + 16
    got = planner(MARG, reqs, budget=budget)
    same(got, expected(MARG, reqs, budget=budget))
    (r,) = got
    assert r["n_lds"] == 3 and list(r["src"]) == [1, 3, 5, 0, 2, 4] and r["ylen_lds"] == 3
    # the sources map back: record i is the record of request src[i] computed alone, but for its place in cols and in the scratch
    for i, k in enumerate(r["src"]):
        (alone,) = planner(MARG, [reqs[k]], budget=budget)
        assert rec_paths(r, i) == rec_paths(alone, 0) and list(r["recs"][i][4:7]) == list(alone["recs"][0][4:7])
    # scratch slices: multiples of 16 bytes, disjoint, in request order, and the total is what the round reports
    ylen = r["recs"][3:, 1] + r["recs"][3:, 3]
    assert list(ylen) == [12, 7, 13]
    start = r["recs"][3:, 7] * 16
    size = -(-ylen * ENTRY // 16) * 16
    assert np.all(size >= ylen * ENTRY) and np.all(size % 16 == 0)
    assert list(start) == [0, size[0], size[0] + size[1]] and r["scr_bytes"] == size.sum()
    assert np.all(r["recs"][:3, 7] == 0)


def test_path_cap_of_one_int(planner):
    # one request per round -- but a record without columns adds no ints, so it does not close its round
    reqs = [gate(0, 1, 1), gate(None, None, 2), gate(None, None, 3), gate(3, None, 4), gate(None, 5, 5), gate(None, None, 6)]
    got = planner(GATE, reqs, path_cap=1)
    same(got, expected(GATE, reqs, path_cap=1))
    assert [list(r["src"]) for r in got] == [[0], [1, 2, 3], [4], [5]]
    reqs = [marg(0, 0), marg(3, 0), marg(11, 11)]
    got = planner(MARG, reqs, path_cap=1)
    same(got, expected(MARG, reqs, path_cap=1))
    assert [r["m"] for r in got] == [1, 1, 1] and all(r["recs"][0][0] == 0 for r in got)     # every round counts its columns from 0


def test_path_cap_is_tested_before_a_request_is_added(planner):
    reqs = [marg(0, 0), marg(3, 0), marg(9, 9), marg(10, 10)]       # 7, 12, 2, 2 ints
    got = planner(MARG, reqs, path_cap=8)
    same(got, expected(MARG, reqs, path_cap=8))
    assert [list(r["src"]) for r in got] == [[0, 1], [2, 3]] and len(got[0]["cols"]) == 19     # 7 < 8: the second joins, 19 >= 8: the round ends
    got = planner(MARG, reqs, path_cap=7)
    assert [list(r["src"]) for r in got] == [[0], [1], [2, 3]]


def test_scratch_cap_cuts_a_round(planner):
    reqs = [marg(8, 8), marg(0, 0), marg(7, 7), marg(3, 0), marg(6, 6), marg(0, 1)]
    budget = 288 + 4 * ENTRY + 16                                    # 7, 12 and 13 entries go to scratch: 2160, 3696, 4016 bytes
    # a round that holds 2160 bytes has reached a cap of 2160, not one of 2161; LDS requests add nothing and never end a round
    for cap, want in ((2160, [[0, 1], [2, 3], [4, 5]]), (2161, [[0, 2, 1, 3], [4, 5]]), (1, [[0, 1], [2, 3], [4, 5]]), (BIG, [[0, 2, 4, 1, 3, 5]])):
        got = planner(MARG, reqs, budget=budget, scratch_cap=cap)
        same(got, expected(MARG, reqs, budget=budget, scratch_cap=cap))
        assert [list(r["src"]) for r in got] == want, cap
        assert all(r["recs"][r["n_lds"]:, 7].min(initial=0) == 0 for r in got)     # every round's slices start at 0


@pytest.mark.parametrize("path_cap,scratch_cap,budget", [(1, BIG, 60 * 1024), (20, BIG, 288 + 16 + 308 * 8), (BIG, 4000, 288 + 16 + 308 * 2),
                                                         (30, 3000, 288 + 16 + 308 * 7), (BIG, BIG, 0)])
def test_every_request_is_in_exactly_one_round(planner, path_cap, scratch_cap, budget):
    rng = np.random.default_rng(7)
    reqs = [marg(int(a), int(b)) for a, b in rng.integers(0, 12, size=(40, 2))]
    got = planner(MARG, reqs, budget=budget, path_cap=path_cap, scratch_cap=scratch_cap)
    same(got, expected(MARG, reqs, budget=budget, path_cap=path_cap, scratch_cap=scratch_cap))
    assert sorted(int(k) for r in got for k in r["src"]) == list(range(40))
    flat = [int(k) for r in got for k in sorted(r["src"])]
    assert flat == list(range(40))                                    # rounds are consecutive runs of the requests
    assert len(got) > 1 or (path_cap == BIG and scratch_cap == BIG)
