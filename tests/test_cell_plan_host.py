"""-m "not gpu": the chunk plan of compute_cell_kzg_proofs_at and recover_cells_and_kzg_proofs_at (kzg_rust_amd/csrc/cell_plan.h: what
cell_proofs_at.hip: cq_run and cell_recover_at.hip: ra_run queue per launch set) run on the CPU, as the stand-alone program
tests/native/cell_plan_probe.cpp under AddressSanitizer and UndefinedBehaviorSanitizer (a child process; nothing is loaded into Python).  For
every layout of tests/cells_at_layout_cases.py, both calls and both forms, the plan is compared with a restatement of the documented rule
 written here from the units alone: a chunk takes whole units, a good unit that would pass CQ_CHUNK pairs closes it, a
unit the host refuses takes slots and no pairs, at most CC_CHUNK units; the pairs of a chunk are numbered in unit order; a pair's slot is its
slot in the chunk (device form) or its own number (host form); the output runs are the maximal runs of filled slots; a recover chunk numbers
its distinct index sets as they come and copies in the known cells of the accepted units only, run of neighbours by run."""
import json
import os
import subprocess

import pytest

import cells_at_layout_cases as lay

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "cell_plan_probe.cpp")
TABLES = 8 * 320                                                   # sizeof(FakeTables) of the probe
REFUSED = 2                                                        # the err word of a unit the host refuses (any word is its BADARGS)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cell_plan") / "cell_plan_probe")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, SRC], check=True)

    def run(numbers):
        r = subprocess.run([exe], input=" ".join(str(v) for v in numbers), capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr
        return [json.loads(ln) for ln in r.stdout.splitlines()]
    return run


def every_call():
    for call in lay.CALLS:
        for name in list(lay.NAMED) + ["msm_%d" % t for t in lay.MSM_TOTALS]:
            yield "%s %s" % (call, name), call, lay.layout(call, name)
        for seed in lay.FUZZ_SEEDS[call]:
            yield "%s fuzz %d" % (call, seed), call, lay.fuzz(call, seed)
        for middle in ("ragged", "refused_at_border"):
            units = lay.replicas_call(call, middle)
            yield "%s replicas %s" % (call, middle), call, units
            for lo, n in lay.ranges(len(units), 3):                # what the driver of one replica is handed
                yield "%s replicas %s from %d" % (call, middle, lo), call, units[lo:lo + n]


CASES = list(every_call())


def mask_of(known):
    return [sum(1 << k for k in known if k < 64), sum(1 << (k - 64) for k in known if k >= 64)]


def restated(call, units, device):
    """the launch sets of a call from the documented rule: one dict per chunk with the keys the probe prints"""
    out, k_before = [], 0                                          # (the call's known cells before the chunk)
    for c0, m, n_pairs, n_slots in lay.split(units):
        chunk = units[c0:c0 + m]
        pairs, first_pair, slot = [], [], 0
        for b, u in enumerate(chunk):
            first_pair.append(len(pairs))
            if not u.host:
                pairs += [[b, k, slot + j if device else len(pairs) + j] for j, k in enumerate(u.want)]
            slot += len(u.want)
        # the runs: maximal runs of filled slots; the pairs are in slot order, so a slot's pair is its rank among the filled ones
        filled = [s for b, u in enumerate(chunk) if not u.host for s in range(sum(len(v.want) for v in chunk[:b]), sum(len(v.want) for v in chunk[:b + 1]))]
        runs = []
        for rank, s in enumerate(filled):
            if runs and runs[-1][1] + runs[-1][2] == s:
                runs[-1][2] += 1
            else:
                runs.append([rank, s, 1])
        want = {"c0": c0, "m": m, "pairs": n_pairs, "slots": n_slots, "any_refused": int(any(u.host for u in chunk)), "pair_list": pairs, "runs": runs,
                "first_pair": first_pair, "refused": [REFUSED if u.host else 0 for u in chunk]}
        assert len(pairs) == n_pairs and slot == n_slots
        if call == "recover":
            cap = min(len(units) - c0, lay.CC_CHUNK)
            seen, sets, first, copies, masks, known, staged = [], [], [], [], [], 0, 0
            for b, u in enumerate(chunk):
                if u.host:
                    sets.append(-1), first.append(0), masks.append(None)
                else:
                    mk = mask_of(u.known)
                    if mk not in seen:
                        seen.append(mk)
                    sets.append(seen.index(mk)), first.append(known if device else staged), masks.append(mk)
                    if not device:
                        if b and not chunk[b - 1].host:
                            copies[-1][1] += len(u.known)
                        else:
                            copies.append([k_before + known, len(u.known)])
                        staged += len(u.known)
                known += len(u.known)
            want.update({"set": sets, "first": first, "copies": copies, "masks": masks, "n_sets": len(seen), "blobs": m, "known": known, "staged": staged,
                         "up_bytes": 16 * cap + 16 * cap, "offsets": [TABLES * cap, TABLES * cap + 16 * cap, TABLES * cap + 32 * cap]})
            k_before += known
        out.append(want)
    return out


def probe_input(call, units, device):
    nums = [lay.CALLS.index(call), int(device), len(units), lay.CC_CHUNK, lay.CQ_CHUNK]
    for u in units:
        if call == "recover":
            nums += [len(u.known)] + list(u.known)
        nums += [len(u.want)] + list(u.want)
    return nums


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("label,call,units", CASES, ids=[c[0] for c in CASES])
def test_the_plan_of_every_layout(probe, label, call, units, device):
    got = probe(probe_input(call, units, device))
    want = restated(call, units, device)
    assert [(g["c0"], g["m"], g["pairs"], g["slots"]) for g in got] == lay.split(units)
    k_before = 0
    for g, w in zip(got, want):
        for key in w:
            assert g[key] == w[key], (label, g["c0"], key)
        chunk = units[g["c0"]:g["c0"] + g["m"]]
        slot_of_unit = [sum(len(v.want) for v in chunk[:b]) for b in range(len(chunk) + 1)]
        # every pair's slot: its slot in the chunk (device form), its own number (host form)
        for p, (b, k, s) in enumerate(g["pair_list"]):
            j = p - g["first_pair"][b]
            assert not chunk[b].host and chunk[b].want[j] == k and s == (slot_of_unit[b] + j if device else p)
        # the runs are maximal, cover the pairs in order, and break exactly where a unit the host refused has slots between good ones
        assert sum(r[2] for r in g["runs"]) == g["pairs"] and [r[0] for r in g["runs"]] == [sum(r[2] for r in g["runs"][:i]) for i in range(len(g["runs"]))]
        holes = [(slot_of_unit[b], slot_of_unit[b + 1]) for b, u in enumerate(chunk) if u.host and u.want]
        for r0, r1 in zip(g["runs"], g["runs"][1:]):
            gap = (r0[1] + r0[2], r1[1])
            assert gap[0] < gap[1] and [h for h in holes if gap[0] <= h[0] and h[1] <= gap[1]] and \
                sum(h[1] - h[0] for h in holes if gap[0] <= h[0] and h[1] <= gap[1]) == gap[1] - gap[0]
        for _, s, n in g["runs"]:
            assert not [h for h in holes if h[0] < s + n and s < h[1]]
        if call == "recover":
            # the copy runs cover exactly the accepted units' known cells, in order
            cells = [c for first, n in g["copies"] for c in range(first, first + n)]
            at, accepted = k_before, []
            for u in chunk:
                if not u.host:
                    accepted += range(at, at + len(u.known))
                at += len(u.known)
            assert cells == ([] if device else accepted) and g["staged"] == len(cells)
            k_before = at


def test_rc_mask_at_its_borders(probe):
    def mask(idx):
        return probe([2, len(idx)] + list(idx))[0]
    for n in (63, 64, 128, 129):
        assert mask(range(n))["ok"] == int(64 <= n <= 128), n
    assert mask(range(64)) == {"ok": 1, "mask": [2 ** 64 - 1, 0]} and mask(range(128)) == {"ok": 1, "mask": [2 ** 64 - 1, 2 ** 64 - 1]}
    assert mask(list(range(63)) + [127]) == {"ok": 1, "mask": [2 ** 63 - 1, 1 << 63]}
    assert mask(list(range(63)) + [128])["ok"] == 0
    assert mask(range(64, 128)) == {"ok": 1, "mask": [0, 2 ** 64 - 1]} and mask(list(range(65, 128)) + [128])["ok"] == 0      # index 127 last; 128
    assert mask([63, 64] + list(range(66, 128))) == {"ok": 1, "mask": [1 << 63, 2 ** 64 - 1 - 2]}                      # the word border
    assert mask(list(range(62)) + [70, 70])["ok"] == 0 and mask(list(range(62)) + [71, 70])["ok"] == 0                  # an equal pair, a descending pair
    assert mask(list(range(62)) + [70, 71])["ok"] == 1


def test_sum_counts_at_the_edge_of_size_t(probe):
    top = (2 ** 64 - 1) // 2048
    assert probe([3, 3, top - 5, 2, 3])[0] == {"ok": 1, "total": top}      # just fits: 2048 * total stays a size_t
    assert probe([3, 3, top - 5, 2, 4])[0]["ok"] == 0                      # passes SIZE_MAX / 2048 at the last count
    assert probe([3, 2, 2 ** 64 - 1, 1])[0]["ok"] == 0 and probe([3, 0])[0] == {"ok": 1, "total": 0}
