"""What tests/test_gpu_cell_sets_device.py adds to the calls of tests/cell_sets_cases.py for verify_cell_kzg_proof_batch_many_sets_device: calls
whose group sizes only the ragged device preparation (k_cell_prep_sets) tells apart, calls of 2 and 3 groups of different lengths for the two
transcript kernels, the upload of a call's four arrays, and the CPU's answer for a group too large for its three sums."""
import cell_batch_cases as bc
import cell_sets_cases as sets

# groups of up to SUMS_UPTO cells are compared with the CPU in all 176 bytes; above, the CPU gives r and [I(tau)]_1 and LL / RL are compared
# between the routes (the rule of tests/test_gpu_cell_batch_shapes.py at its largest sizes)
SUMS_UPTO = 4096

SORT_TILES = [2048, 2049, 1]          # the second CP_SORT_TILE of the column placement, and a one-cell group behind it
TABLES = [4096, 4097, 3]              # the fullest LDS dedup table, the first HBM one, and a tiny group behind the HBM one
OVER_THE_CAP = [16385, 2]             # one group above CELL_PREP_MAX_CELLS: the host prepares the whole call


def sized(pools, name, sizes):
    """groups of the given sizes: the large ones as tests/test_gpu_cell_batch_shapes.py builds them (setup points as commitments: well-formed,
    False; neighbours share commitments, which must not merge), the small ones valid cuts of the mixed pool"""
    groups = []
    for t, n in enumerate(sizes):
        if n > 16384:
            groups.append(bc.setup_group(pools, n, every=2))
        elif n > 256:
            groups.append(bc.setup_group(pools, n))
        else:
            groups.append(sets.cut(pools, f"{name}-tail{t}", 310 + 10 * t, n))
    spoiled = {t: "spoiled" for t, n in enumerate(sizes) if n > 256}
    share = [(t, t + 1) for t in range(len(sizes) - 1) if sizes[t] > 256 and sizes[t + 1] > 256]      # both start at the first setup point
    return sets.Call(name, groups, sizes, share_commitment=share, spoiled=spoiled)


def hash_calls(pools):
    """2 and 3 groups, all of different lengths: on a handle with rhash_lanes_from = 3 the wave kernel hashes the first call, the lane kernel the second"""
    two = sets.Call("hash-2", [sets.cut(pools, "hash2a", 400, 9), sets.cut(pools, "hash2b", 409, 2)], [9, 2])
    three = sets.Call("hash-3", [sets.cut(pools, "hash3a", 420, 3), sets.cut(pools, "hash3b", 423, 70), sets.cut(pools, "hash3c", 493, 1)], [3, 70, 1])
    return [two, three]


def flat(groups):
    """(commitments, cell indices, cells, proofs) of a call as the four arrays of the C interface, and the counts"""
    return (b"".join(b"".join(g.c) for g in groups), [int(i) for g in groups for i in g.i], b"".join(b"".join(g.cells) for g in groups),
            b"".join(b"".join(g.p) for g in groups), [g.n for g in groups])


def to_device(torch, groups, shift=0):
    """the four arrays as device tensors (None for a call without a cell); shift: bytes by which the commitments are moved off their allocation's
    start (a view into a larger tensor: a misaligned bulk pointer when shift is no multiple of 16)"""
    c, idx, cells, p, _ = flat(groups)
    if not idx:
        return None, None, None, None
    u8 = lambda data: torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()      # noqa: E731
    dc = u8(bytes(shift) + c)[shift:]
    return dc, torch.tensor(idx, dtype=torch.int64).cuda(), u8(cells), u8(p)


def cpu_answer(reference, g):
    """(verdict or "BadArgs" or None, r | [I(tau)]_1 | LL | RL or None, compared bytes): all 176 bytes up to SUMS_UPTO cells, the first 80 above
    (verdict None: the CPU has not added the group's points up)"""
    if g.n <= SUMS_UPTO:
        verdict, raw = sets.cpu_answer(reference, g)
        return verdict, raw, 176
    r, itau, _, _, _ = reference(*g.args, sums=False)
    return None, r + itau, 80
