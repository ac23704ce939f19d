"""The call layouts of tests/test_gpu_cells_at_layouts.py: ragged calls of compute_cell_kzg_proofs_at_many and
recover_cells_and_kzg_proofs_at_many_sets whose units sit at the borders of the launch sets that cell_proofs_at.hip: cq_run and
cell_recover_at.hip: ra_run cut them into, with the chunk rule of those two loops restated (split) and the answer of every call (expected).
Pinned on the CPU by tests/test_cells_at_layout_cases.py.  A unit is fixture blob i % 3 of tests/golden/cells.json with a seeded want list
and, for the recovery, the known set that is next in recover_at_cases.index_sets(); the expected bytes of every accepted unit come from
recover_at_cases.fixture() (cells from cell_spec.compute_cells, proofs oracle-derived), never from a library call.  No GPU import here."""
import functools
import os
import random
import re
import typing

import recover_at_cases as rc

HERE = os.path.dirname(os.path.abspath(__file__))
ENGINE_H = open(os.path.join(HERE, "..", "kzg_rust_amd", "csrc", "engine.h")).read()
CQ_CHUNK = int(re.search(r"CQ_CHUNK = (\d+);", ENGINE_H).group(1))      # (blob, cell) pairs per launch set
CC_CHUNK = int(re.search(r"CC_CHUNK = (\d+);", ENGINE_H).group(1))      # units per launch set
R = rc.R
CELL, BLOB, BADARGS = 2048, 131072, 1
CALLS = ("compute", "recover")
DEVICE = "element equal to r"                                      # the one refusal the device makes: the host counts the unit's pairs
HOST_KINDS = {"compute": ("count of 129", "wanted index 128"),
              "recover": ("63 known cells", "129 known cells", "known indices not ascending", "wanted index 128", "129 wanted")}
SETS64 = (0, 1, 2, 3, 4)                                           # the 64-cell sets of index_sets(): what a layout of hundreds of units cycles through
FUZZ_COUNTS = (0, 1, 2, 7, 64, 127, 128)
# eight seeds per call, found by search over the model alone: the last four split into two launch sets, the last with a refused unit at the border
FUZZ_SEEDS = {"compute": (1, 2, 5, 8, 3, 20, 49, 205), "recover": (3, 5, 6, 8, 45, 55, 86, 567)}


class Unit(typing.NamedTuple):
    b: int                  # fixture blob
    known: tuple            # recover: the known indices as the call gets them; compute: ()
    want: tuple             # the want list as the call gets it: its length is the unit's slots
    refusal: typing.Optional[str]
    spoil: tuple            # DEVICE: (element of the blob,) for compute, (known cell, element of it) for recover

    @property
    def host(self):
        """refused by the host's own checks: slots and no pairs"""
        return self.refusal is not None and self.refusal != DEVICE


def make_unit(call, i, count, refusal, rng, small_sets=False):
    """unit i of a layout: `count` wanted cells (for a host refusal: slots), refused as `refusal` says"""
    assert call in CALLS and (refusal is None or refusal == DEVICE or refusal in HOST_KINDS[call]), (call, refusal)
    b = i % 3
    want = [rng.randrange(128) for _ in range(count)]
    known, spoil = (), ()
    if call == "recover":
        sets = rc.index_sets()
        known = list(sets[SETS64[i % 5] if small_sets else i % 9][1])
        if refusal == "63 known cells":
            known = known[:63]
        elif refusal == "129 known cells":
            known = list(range(128)) + [128]
        elif refusal == "known indices not ascending":
            j = rng.randrange(len(known) - 1)
            known[j], known[j + 1] = known[j + 1], known[j]
    if refusal == "wanted index 128":
        assert count > 0
        want[rng.randrange(count)] = 128
    if refusal in ("count of 129", "129 wanted"):
        assert count == 129
    if refusal == DEVICE:
        spoil = (rng.randrange(4096),) if call == "compute" else (rng.randrange(len(known)), rng.randrange(64))
    return Unit(b, tuple(known), tuple(want), refusal, spoil)


def build(call, spec, seed, small_sets=False):
    """units from a list of want counts; ("H", slots, kind) is a unit the host refuses, ("D", count) one the device refuses"""
    rng = random.Random(seed)
    units = []
    for i, e in enumerate(spec):
        if isinstance(e, int):
            units.append(make_unit(call, i, e, None, rng, small_sets))
        elif e[0] == "H":
            units.append(make_unit(call, i, e[1], e[2], rng, small_sets))
        else:
            units.append(make_unit(call, i, e[1], DEVICE, rng, small_sets))
    return units


# ---- the chunk model
def split(units):
    """[(first unit, units, pairs, slots)] of the launch sets of a call, the rule of cq_run / ra_run restated: a chunk takes whole units; a good
    unit that would pass CQ_CHUNK pairs closes it; a unit the host refuses adds slots and no pairs and never closes it; at most CC_CHUNK units"""
    out, c0 = [], 0
    while c0 < len(units):
        m = pairs = slots = 0
        while c0 + m < len(units) and m < CC_CHUNK:
            u = units[c0 + m]
            if not u.host and pairs + len(u.want) > CQ_CHUNK:
                break
            pairs += 0 if u.host else len(u.want)
            slots += len(u.want)
            m += 1
        out.append((c0, m, pairs, slots))
        c0 += m
    return out


def ranges(n, devices):
    """the contiguous ranges of n units over the replicas of a handle (multi_device.hip: fan_out): [(first unit, units)], empty ones left out"""
    d = min(n, devices)
    cuts = [n * k // d for k in range(d + 1)]
    return [(lo, hi - lo) for lo, hi in zip(cuts, cuts[1:]) if hi > lo]


# ---- the answer model
def expected(units):
    """(statuses, cells_out bytes, proofs_out bytes, [(first slot, end slot)] of the refused units): the bytes of an accepted unit are the
    fixture's; a refused unit's slots are unspecified and are zeros here (blank() makes a call's outputs comparable)"""
    fx = rc.fixture()
    statuses, c, p, holes, slot = [], [], [], [], 0
    for u in units:
        n = len(u.want)
        statuses.append(BADARGS if u.refusal else 0)
        if u.refusal:
            c.append(bytes(CELL * n))
            p.append(bytes(48 * n))
            if n:
                holes.append((slot, slot + n))
        else:
            c.extend(fx["cells"][u.b][k] for k in u.want)
            p.extend(fx["P"][u.b][k] for k in u.want)
        slot += n
    return statuses, b"".join(c), b"".join(p), holes


def blank(buf, holes, width):
    """buf with the slots of the refused units zeroed"""
    out = bytearray(buf)
    for lo, hi in holes:
        out[width * lo:width * hi] = bytes(width * (hi - lo))
    return bytes(out)


# ---- what the calls take
def blob_of(u):
    """compute: the unit's blob"""
    blob = rc.fixture()["blobs"][u.b]
    if u.refusal == DEVICE:
        e, = u.spoil
        blob = blob[:32 * e] + R.to_bytes(32, "big") + blob[32 * e + 32:]
    return blob


def known_cells_of(u):
    """recover: the unit's known cells, one per entry of u.known (index 128 brings cell 0, as in recover_at_cases.refusals)"""
    cells = rc.fixture()["cells"][u.b]
    out = [cells[k % 128] for k in u.known]
    if u.refusal == DEVICE:
        at, e = u.spoil
        out[at] = out[at][:32 * e] + R.to_bytes(32, "big") + out[at][32 * e + 32:]
    return out


def call_arrays(call, units):
    """(input bytes, known counts or None, known indices or None, want counts, want indices): the input is the blobs of a compute call, the known
    cells of a recovery"""
    wc, wi = [len(u.want) for u in units], [k for u in units for k in u.want]
    if call == "compute":
        return b"".join(blob_of(u) for u in units), None, None, wc, wi
    return (b"".join(b"".join(known_cells_of(u)) for u in units), [len(u.known) for u in units], [k for u in units for k in u.known], wc, wi)


# ---- the named layouts
NAMED = ("ragged", "riders", "refused_at_border", "unit_border", "empty_chunk_first")
MSM_TOTALS = (15, 16, 127, 128, 1023, 1024)                      # one below and at every border of msm_wide_shape
MSM_COUNTS = {15: [7, 0, 8], 16: [1, 8, 7], 127: [64, 0, 63], 128: [100, 27, 1], 1023: [128] * 7 + [100, 27], 1024: [128] * 7 + [64, 1, 63]}
# the launch sets the model must give: (units, pairs, slots)
CHUNKS = {"ragged": [(9, 1124, 1124), (5, 194, 194)], "riders": [(12, 1152, 1152), (2, 4, 4)],
          "refused_at_border": [(12, 1152, 1284), (4, 14, 14)], "unit_border": [(512, 510, 514), (4, 1, 5)],
          "empty_chunk_first": [(512, 0, 0), (1, 3, 3)]}


@functools.lru_cache(maxsize=None)
def layout(call, name):
    """the units of a named layout; "msm_<total>" is the single-chunk call of msm_borders with that many pairs"""
    compute = call == "compute"
    seed = "%s %s" % (call, name)
    if name == "ragged":
        return build(call, [128] * 8 + [100, 60, 5, 0, 128, 1], seed)
    if name == "riders":
        return build(call, [128] * 8 + [127, 1, 0, ("D", 0), 1, 3], seed)
    if name == "refused_at_border":
        h129 = "count of 129" if compute else "129 wanted"
        h3 = "wanted index 128" if compute else "129 known cells"      # (129 known cells move the known-cell offset by 129)
        return build(call, [128] * 8 + [120, ("H", 129, h129), 8, ("H", 3, h3), ("D", 5), 7, 0, 2], seed)
    if name == "unit_border":
        kinds = ["wanted index 128"] * 4 if compute else ["63 known cells", "129 known cells", "known indices not ascending", "wanted index 128"]
        spec = [i % 3 for i in range(516)]
        for i, kind in zip((0, 511, 512, 515), kinds):
            spec[i] = ("H", 2, kind)
        return build(call, spec, seed, small_sets=True)
    if name == "empty_chunk_first":
        return build(call, [0] * 512 + [3], seed, small_sets=True)
    total = int(re.fullmatch(r"msm_(\d+)", name).group(1))
    return build(call, MSM_COUNTS[total], seed)


def replicas_call(call, middle):
    """[a unit wanting 3] + ragged, `middle`, ragged + [a unit wanting 9]: over three replicas every range runs in two launch sets"""
    ends = build(call, [3, 9], "%s replicas" % call)
    return [ends[0]] + layout(call, "ragged") + layout(call, middle) + layout(call, "ragged") + [ends[1]]


# ---- the fuzz layouts
@functools.lru_cache(maxsize=None)
def fuzz(call, seed):
    """1..24 units with want counts out of FUZZ_COUNTS; about one in six is refused, of a random kind"""
    rng = random.Random("%s fuzz %d" % (call, seed))
    kinds = HOST_KINDS[call] + (DEVICE,)
    spec = []
    for _ in range(rng.randint(1, 24)):
        count = rng.choice(FUZZ_COUNTS)
        if rng.randrange(6):
            spec.append(count)
            continue
        kind = rng.choice(kinds)
        if kind == DEVICE:
            spec.append(("D", count))
        else:
            spec.append(("H", 129 if kind in ("count of 129", "129 wanted") else max(count, 1) if kind == "wanted index 128" else count, kind))
    return build(call, spec, "%s fuzz units %d" % (call, seed))


def refused_at_the_border(units):
    """a refused unit is the last of launch set 0 or the first of launch set 1"""
    chunks = split(units)
    return len(chunks) > 1 and (units[chunks[0][1] - 1].refusal is not None or units[chunks[1][0]].refusal is not None)
