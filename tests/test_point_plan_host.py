"""-m "not gpu": the chunk plan of compute_kzg_proofs_at (kzg_rust_amd/csrc/point_plan.h: what point_proofs_at.hip: pq_run queues per launch
set) run on the CPU, as the stand-alone program tests/native/point_plan_probe.cpp, built plain and under AddressSanitizer and
UndefinedBehaviorSanitizer (a child process; nothing is loaded into Python).  The plan is compared with a restatement of the documented rule
 written here from the counts alone: a chunk takes pieces of blobs in blob order, at most CC_CHUNK of them and CQ_CHUNK
pairs; a piece is the whole blob while its points fit, the blob at the border is cut there and the next chunk starts with the rest of it; a
blob the host refuses (more than 4096 points, or a point >= r) and a blob that wants nothing take a piece without pairs, so they ride behind
a full chunk's last pair; a pair's slot is the call's slot (device form) or its own number (host form); the output runs are the maximal runs
of filled slots."""
import json
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "point_plan_probe.cpp")
CC_CHUNK, CQ_CHUNK = 512, 1152                                     # engine.h
REFUSED = 2                                                        # the err word of a blob the host refuses (any word is its BADARGS)
R_AT, FF_AT = 1, 5000                                              # the probe's bad-point codes: 1 + j: point j = r, 5000 + j: 32 x 0xff


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def probe(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("point_plan") / "point_plan_probe")
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.run(["g++", "-std=c++17"] + flags + ["-o", exe, SRC], check=True)

    def run(numbers):
        r = subprocess.run([exe], input=" ".join(str(v) for v in numbers), capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr
        return [json.loads(ln) for ln in r.stdout.splitlines()]
    return run


def good(count, bad):
    return count <= 4096 and not bad


def restated(blobs, device, max_units=CC_CHUNK, max_pairs=CQ_CHUNK):
    """the launch sets of a call over blobs = [(count, bad)]: one dict per chunk with the keys the probe prints"""
    first = [sum(c for c, _ in blobs[:i]) for i in range(len(blobs))]
    out, b, done = [], 0, 0
    while b < len(blobs):
        pieces, pairs, points = [], [], []
        while b < len(blobs) and len(pieces) < max_units:
            count, bad = blobs[b]
            left = count - done if good(count, bad) else 0
            room = max_pairs - len(pairs)
            if left and not room:
                break
            take = min(left, room)
            pieces.append([b, done, take, len(pairs), first[b] + done])
            for j in range(take):
                pairs.append([len(pieces) - 1, first[b] + done + j if device else len(pairs)])
                points.append(65536 * b + done + j + 1)
            if take == left:
                b, done = b + 1, 0
            else:
                done += take
                break
        filled = [p[4] + j for p in pieces for j in range(p[2])]
        runs = []
        for rank, s in enumerate(filled):
            if runs and runs[-1][1] + runs[-1][2] == s:
                runs[-1][2] += 1
            else:
                runs.append([rank, s, 1])
        refused = [0 if good(*blobs[p[0]]) else REFUSED for p in pieces]
        out.append({"m": len(pieces), "pairs": len(pairs), "any_refused": int(any(refused)), "pieces": pieces, "pair_list": pairs, "runs": runs,
                    "refused": refused, "points": points})
    return out


def chunk_count(counts):
    """how many launch sets a call of good blobs with these counts takes (tests/test_gpu_point_proofs_at.py counts pq_quotient launches with
    it: the chunks that have a pair)"""
    return sum(1 for c in restated([(k, 0) for k in counts], False) if c["pairs"])


CALLS = {
    "whole_blobs_while_they_fit": [(500, 0), (500, 0), (152, 0), (3, 0), (1149, 0)],
    "one_blob_cut_1152_1": [(1153, 0)],
    "riders_behind_the_tail": [(1153, 0), (1, 0), (0, 0), (5, 0)],
    "cut_in_the_middle_of_a_call": [(7, 0), (1150, 0), (4096, 0), (2, 0)],
    "refused_first_and_last_in_a_chunk": [(9, R_AT + 8), (1152, 0), (4, R_AT), (3, FF_AT + 1), (1152, 0), (2, FF_AT)],
    "refused_between_pieces": [(1000, 0), (4097, 0), (300, R_AT + 299), (200, 0)],
    "512_blobs": [(1, 0)] * 512,
    "513_blobs": [(1, 0)] * 513,
    "a_chunk_with_no_pair": [(0, 0)] * 512 + [(3, 0)],
    "zero_counts_behind_a_full_chunk": [(1152, 0), (0, 0), (0, 0), (1, 0)],
    "counts_0_and_4096": [(0, 0), (4096, 0), (0, 0)],
    "4097_refused": [(4097, 0), (2, 0)],
    "4096_with_the_last_point_bad": [(4096, R_AT + 4095), (1, 0)],
    "nothing_wanted_at_all": [(0, 0), (0, 0)],
}


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", list(CALLS))
def test_the_plan_of_every_call(probe, name, device):
    blobs = CALLS[name]
    nums = [0, int(device), len(blobs), CC_CHUNK, CQ_CHUNK]
    for count, bad in blobs:
        nums += [count, bad if count <= 4096 else 0]
    got, want = probe(nums), restated(blobs, device)
    assert len(got) == len(want), name
    for g, w in zip(got, want):
        for key in w:
            assert g[key] == w[key], (name, key)
    # what the rule promises, on the probe's output alone: every good blob's points are taken once, in order; no chunk passes its caps
    taken = {}
    for g in got:
        assert 0 < g["m"] <= CC_CHUNK and g["pairs"] <= CQ_CHUNK
        for b, skip, n, _, _ in g["pieces"]:
            assert skip == taken.get(b, 0)
            taken[b] = skip + n
    assert taken == {b: (c if good(c, bad) else 0) for b, (c, bad) in enumerate(blobs)}


def test_the_named_shapes_cut_where_the_rule_says(probe):
    sizes = lambda blobs: [(g["m"], g["pairs"]) for g in probe([0, 0, len(blobs), CC_CHUNK, CQ_CHUNK] + [v for cb in blobs for v in cb])]      # noqa: E731
    assert sizes(CALLS["one_blob_cut_1152_1"]) == [(1, 1152), (1, 1)]
    assert sizes(CALLS["riders_behind_the_tail"]) == [(1, 1152), (4, 7)]
    assert sizes(CALLS["512_blobs"]) == [(512, 512)] and sizes(CALLS["513_blobs"]) == [(512, 512), (1, 1)]
    assert sizes(CALLS["a_chunk_with_no_pair"]) == [(512, 0), (1, 3)]
    assert sizes(CALLS["counts_0_and_4096"]) == [(2, 1152), (1, 1152), (1, 1152), (2, 640)]
    assert sizes(CALLS["4097_refused"]) == [(2, 2)]
    assert chunk_count([1153, 1, 0, 5]) == 2 and chunk_count([1] * 513) == 2 and chunk_count([0] * 512 + [3]) == 1


def test_small_caps_cut_every_blob(probe):
    blobs = [(5, 0), (0, 0), (7, R_AT), (11, 0), (1, 0)]
    for units, pairs in ((2, 3), (1, 100), (3, 1)):
        for device in (False, True):
            nums = [0, int(device), len(blobs), units, pairs] + [v for cb in blobs for v in cb]
            assert probe(nums) == restated(blobs, device, units, pairs), (units, pairs, device)


def test_points_are_compared_with_r_byte_for_byte(probe):
    assert [probe([2, which])[0]["ok"] for which in range(5)] == [1, 0, 0, 1, 0]      # r - 1, r, r + 1, 0, 32 x 0xff


def test_sum_point_counts_at_the_edge_of_size_t(probe):
    top = (2 ** 64 - 1) // 48
    assert probe([1, 3, top - 5, 2, 3])[0] == {"ok": 1, "total": top}      # just fits: 48 * total stays a size_t
    assert probe([1, 3, top - 5, 2, 4])[0]["ok"] == 0                      # passes SIZE_MAX / 48 at the last count
    assert probe([1, 2, 2 ** 64 - 1, 1])[0]["ok"] == 0 and probe([1, 0])[0] == {"ok": 1, "total": 0}
