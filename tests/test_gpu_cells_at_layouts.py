"""-m gpu: the launch-set bookkeeping of compute_cell_kzg_proofs_at_many (cell_proofs_at.hip: cq_run) and
recover_cells_and_kzg_proofs_at_many_sets (cell_recover_at.hip: ra_run) at its borders, in the host form, the device form and over replicas:
ragged chunk breaks, units that want nothing at the end of a full chunk, refused units last and first in a chunk, the unit-count border, a
chunk without a pair, the MSM's launch shapes at their exact pair counts, seeded ragged calls, ranges that run in two launch sets each, a
workspace that grows and shrinks, two threads on one handle and the launch counts of the kernel timing.  The calls and their answers are
built on the CPU in tests/cells_at_layout_cases.py (pinned by tests/test_cells_at_layout_cases.py): the expected bytes of every accepted
unit come from the fixture (cells from cell_spec.compute_cells, proofs oracle-derived), never from a library call.  Every call goes through
ctypes; its return value, its statuses by position and every accepted unit's cell and proof slots are compared byte for byte (a refused
unit's slots are unspecified), and every output buffer, host or device, sits between two guards of 4096 bytes that must come back intact."""
import ctypes as C
import os
import threading

import pytest

import cells_at_layout_cases as lay
import recover_at_cases as rc

pytestmark = pytest.mark.gpu

CELL, BADARGS = lay.CELL, lay.BADARGS
GUARD, GUARD_BYTE, FILL_BYTE = 4096, 0xA5, 0x3C                  # (4096 keeps a device pointer behind the guard 16-byte aligned)
BORDERS = ("ragged", "riders", "refused_at_border")
BIG = ("unit_border", "empty_chunk_first")
OUTPUTS = ((True, True), (True, False), (False, True))           # (cells, proofs)
PER_CHUNK_FAMILY = {"compute": "cc_field", "recover": "rc_interp"}


@pytest.fixture(scope="module")
def kz():
    import kzg_rust_amd
    return kzg_rust_amd


def _load(kz, setup_bytes, **options):
    g1, g2 = setup_bytes
    return kz.KzgSettings.load_trusted_setup_ex([g1[48 * i:48 * i + 48] for i in range(4096)], [g2[96 * i:96 * i + 96] for i in range(65)], **options)


@pytest.fixture(scope="module")
def s8(kz, setup_bytes):
    """bucket form, no table: the MSM's digits come from launch_digits_from_fr"""
    s = _load(kz, setup_bytes, msm_bits=8)
    yield s
    s.free()


@pytest.fixture(scope="module")
def s12(kz, setup_bytes):
    """the smallest wide table: the MSM is the scalar-input instance of k_msm_wide"""
    s = _load(kz, setup_bytes, msm_bits=12)
    yield s
    s.free()


@pytest.fixture(scope="module", params=["bucket", "wide"])
def handle(request, s8, s12):
    return s8 if request.param == "bucket" else s12


@pytest.fixture(scope="module")
def s3(kz, setup_bytes):
    """three replicas of device 0, loaded as tests/test_gpu_cell_proofs_at.py::test_replicas loads them"""
    g1, g2 = setup_bytes
    env = dict(KZG355_MSM="bucket", KZG355_EXCHANGE="peer")     # no wide table per replica
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        s = kz.Kzg.load_trusted_setup([g1[48 * i:48 * i + 48] for i in range(4096)], [g2[96 * i:96 * i + 96] for i in range(65)], devices=[0, 0, 0])
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    yield s
    s.free()


# ---- the two calls through ctypes, between guards
def _sz(v):
    return (C.c_size_t * max(len(v), 1))(*v)


class HostOut:
    def __init__(self, n):
        self.n = n
        self.mem = bytearray(bytes([GUARD_BYTE]) * GUARD + bytes([FILL_BYTE]) * n + bytes([GUARD_BYTE]) * GUARD)
        self.arg = (C.c_char * max(n, 1)).from_buffer(self.mem, GUARD)

    def take(self, what):
        whole = bytes(self.mem)
        assert whole[:GUARD] == bytes([GUARD_BYTE]) * GUARD, "%s: the guard before the host buffer was written" % what
        assert whole[GUARD + self.n:] == bytes([GUARD_BYTE]) * GUARD, "%s: the guard behind the host buffer was written" % what
        return whole[GUARD:GUARD + self.n]


class DeviceOut:
    def __init__(self, torch, n):
        self.n = n
        self.mem = torch.full((GUARD + n + GUARD,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
        self.mem[GUARD:GUARD + n] = FILL_BYTE
        self.arg = self.mem.data_ptr() + GUARD
        assert self.arg % 16 == 0

    def take(self, what):
        whole = bytes(self.mem.cpu().numpy())
        assert whole[:GUARD] == bytes([GUARD_BYTE]) * GUARD, "%s: the guard before the device buffer was written" % what
        assert whole[GUARD + self.n:] == bytes([GUARD_BYTE]) * GUARD, "%s: the guard behind the device buffer was written" % what
        return whole[GUARD:GUARD + self.n]


class Prepared:
    """a call laid out for the C ABI: run() makes it (from any thread), result() checks the guards and, in the device form, that the input
    is as it was, and gives (return value, statuses, cells_out bytes or None, proofs_out bytes or None)"""

    def __init__(self, kz, s, call, units, cells=True, proofs=True, device=False):
        self.call, self.device, self.handle, self.m = call, device, s.handle, len(units)
        self.data, kc, ki, wc, wi = lay.call_arrays(call, units)
        self.arrays = [_sz(v) for v in ((wc, wi) if call == "compute" else (kc, ki, wc, wi))]
        total = len(wi)
        lib = kz.kzg.lib()
        if device:
            import torch
            self.torch = torch
            self.d_in = torch.frombuffer(bytearray(self.data), dtype=torch.uint8).cuda()
            self.input = self.d_in.data_ptr()
            self.c = DeviceOut(torch, CELL * total) if cells else None
            self.p = DeviceOut(torch, 48 * total) if proofs else None
            torch.cuda.synchronize()
            self.fn = lib.kzg355_compute_cell_kzg_proofs_at_many_device if call == "compute" else lib.kzg355_recover_cells_and_kzg_proofs_at_many_sets_device
        else:
            self.input = self.data
            self.c = HostOut(CELL * total) if cells else None
            self.p = HostOut(48 * total) if proofs else None
            self.fn = lib.kzg355_compute_cell_kzg_proofs_at_many if call == "compute" else lib.kzg355_recover_cells_and_kzg_proofs_at_many_sets
        self.st = (C.c_int * max(self.m, 1))(*([7] * max(self.m, 1)))
        self.rc = None

    def run(self):
        c, p = self.c.arg if self.c else None, self.p.arg if self.p else None
        if self.call == "compute":
            counts, idx = self.arrays
            self.rc = self.fn(c, p, self.st, self.input, self.m, counts, idx, self.handle)
        else:
            kc, ki, wc, wi = self.arrays
            self.rc = self.fn(c, p, self.st, kc, ki, self.input, wc, wi, self.m, self.handle)
        return self

    def result(self):
        what = "%s, %s form" % (self.call, "device" if self.device else "host")
        if self.device:
            self.torch.cuda.synchronize()
            assert bytes(self.d_in.cpu().numpy()) == self.data, "%s: the input buffer was changed" % what
        return (self.rc, list(self.st)[:self.m], self.c.take(what + ", cells_out") if self.c else None,
                self.p.take(what + ", proofs_out") if self.p else None)


def run(kz, s, call, units, cells=True, proofs=True, device=False):
    return Prepared(kz, s, call, units, cells, proofs, device).run().result()


# ---- the comparison
_ANSWERS = {}


def answer(units):
    """lay.expected(units), computed once per list of units (the lists are the cases module's own, built once)"""
    if id(units) not in _ANSWERS:
        _ANSWERS[id(units)] = (units, lay.expected(units))
    return _ANSWERS[id(units)][1]


def same_slots(got, exp, width, what):
    """byte-for-byte equality, reported by slot (a failed comparison of megabytes is not to be printed)"""
    assert len(got) == len(exp), "%s: %d bytes for %d" % (what, len(got), len(exp))
    if got != exp:
        bad = [s for s in range(len(exp) // width) if got[width * s:width * (s + 1)] != exp[width * s:width * (s + 1)]]
        raise AssertionError("%s: %d of %d slots differ, the first at %s" % (what, len(bad), len(exp) // width, bad[:12]))


def check(res, units, what, cells=True, proofs=True):
    """the call's return value, its statuses by position and every accepted unit's slots against the model"""
    statuses, exp_c, exp_p, holes = answer(units)
    rcode, st, c, p = res
    assert rcode == (BADARGS if any(statuses) else 0), what
    assert st == statuses, what
    assert (c is not None, p is not None) == (cells, proofs), what
    if cells:
        same_slots(lay.blank(c, holes, CELL), exp_c, CELL, what + ": cells_out")
    if proofs:
        same_slots(lay.blank(p, holes, 48), exp_p, 48, what + ": proofs_out")
    return res


def check_equal(a, b, units, what):
    """two results of the same call agree on everything but the refused units' slots"""
    holes = answer(units)[3]
    assert a[:2] == b[:2], what
    same_slots(lay.blank(a[2], holes, CELL), lay.blank(b[2], holes, CELL), CELL, what + ": cells_out")
    same_slots(lay.blank(a[3], holes, 48), lay.blank(b[3], holes, 48), 48, what + ": proofs_out")


# ---- 1. the pair border in the host form: a ragged break, riders at the end of a full chunk, refused units on both sides of the break
@pytest.mark.parametrize("name", BORDERS)
@pytest.mark.parametrize("call", lay.CALLS)
def test_host_form(kz, handle, call, name):
    units = lay.layout(call, name)
    assert len(lay.split(units)) == 2
    for cells, proofs in OUTPUTS if name == "ragged" else OUTPUTS[:1]:
        check(run(kz, handle, call, units, cells, proofs), units, "%s %s" % (call, name), cells, proofs)


# ---- 2. the same in the device form, where slots, output pointers, proof copies and known cells are chunk-relative
@pytest.mark.parametrize("form,name", [("bucket", n) for n in BORDERS] + [("wide", n) for n in BORDERS + BIG])
@pytest.mark.parametrize("call", lay.CALLS)
def test_device_form(kz, s8, s12, call, form, name):
    handle = s8 if form == "bucket" else s12
    units = lay.layout(call, name)
    assert len(lay.split(units)) == 2
    what = "%s %s" % (call, name)
    dev = check(run(kz, handle, call, units, device=True), units, what)
    host = check(run(kz, handle, call, units), units, what)
    check_equal(dev, host, units, what + ", device against host")
    if name == "ragged":
        for cells, proofs in OUTPUTS[1:]:
            check(run(kz, handle, call, units, cells, proofs, device=True), units, what, cells, proofs)


# ---- 3. the unit border and a chunk without a pair before one with pairs, host form
@pytest.mark.parametrize("name", BIG)
@pytest.mark.parametrize("call", lay.CALLS)
def test_unit_border_host_form(kz, s12, call, name):
    units = lay.layout(call, name)
    assert [c[1] for c in lay.split(units)] == [lay.CC_CHUNK, len(units) - lay.CC_CHUNK]
    check(run(kz, s12, call, units), units, "%s %s" % (call, name))


# ---- 4. the MSM on scalars at the exact borders of its launch shape (k_msm_wide.hip: msm_wide_shape), and the digits of the bucket form
@pytest.mark.parametrize("total", lay.MSM_TOTALS)
@pytest.mark.parametrize("call", lay.CALLS)
def test_msm_borders(kz, handle, s12, call, total):
    units = lay.layout(call, "msm_%d" % total)
    assert [c[2] for c in lay.split(units)] == [total]
    what = "%s, %d pairs" % (call, total)
    check(run(kz, handle, call, units), units, what)
    if handle is s12:
        check(run(kz, s12, call, units, device=True), units, what)


# ---- 5. seeded ragged calls
@pytest.mark.parametrize("k", range(8))
@pytest.mark.parametrize("call", lay.CALLS)
def test_fuzz(kz, handle, s12, call, k):
    seed = lay.FUZZ_SEEDS[call][k]
    units = lay.fuzz(call, seed)
    what = "%s, seed %d" % (call, seed)
    host = check(run(kz, handle, call, units), units, what)
    if handle is s12:
        dev = check(run(kz, s12, call, units, device=True), units, what)
        check_equal(dev, host, units, what + ", device against host")


# ---- 6. replicas: every range of the call runs in two launch sets, and its offsets are those of the range
@pytest.mark.parametrize("middle", ["ragged", "refused_at_border"])
@pytest.mark.parametrize("call", lay.CALLS)
def test_replicas(kz, s8, s3, call, middle):
    assert s3.device_count == 3
    units = lay.replicas_call(call, middle)
    rs = lay.ranges(len(units), 3)
    assert len(rs) == 3 and all(len(lay.split(units[lo:lo + n])) == 2 for lo, n in rs)
    what = "%s replicas, %s in the middle" % (call, middle)
    single = check(run(kz, s8, call, units), units, what + ", one device")
    before = s3.cell_calls_per_device()
    multi = check(run(kz, s3, call, units), units, what)
    assert [a - b for a, b in zip(s3.cell_calls_per_device(), before)] == [1, 1, 1]
    check_equal(multi, single, units, what + ", replicas against one device")


# ---- 7. one workspace through calls that grow and shrink, and its neighbours afterwards
@pytest.mark.parametrize("call", lay.CALLS)
def test_workspace_grows_and_shrinks(kz, setup_bytes, call):
    fx = rc.fixture()
    blobs = [kz.Blob(b) for b in fx["blobs"]]
    ix = rc.index_sets()[5][1]
    raw = lambda xs: [bytes(x) for x in xs]                        # noqa: E731
    s = _load(kz, setup_bytes, msm_bits=12)

    def neighbours():
        cms = raw(kz.Kzg.blob_to_kzg_commitment_many(blobs, s))
        c, p = kz.Kzg.recover_cells_and_kzg_proofs(ix, [fx["cells"][2][k] for k in ix], s)
        cm = kz.KzgCommitment(bytes.fromhex(fx["commitments"][0]))
        ok = kz.Kzg.verify_cell_kzg_proof_batch([cm] * 3, [0, 64, 127], [fx["cells"][0][k] for k in (0, 64, 127)], [fx["P"][0][k] for k in (0, 64, 127)], s)
        return cms, (raw(c), raw(p)), ok

    try:
        before = neighbours()
        assert before == ([bytes.fromhex(x) for x in fx["commitments"]], (fx["cells"][2], fx["P"][2]), True)
        small = lay.layout(call, "msm_15")                         # 3 units
        assert len(small) == 3
        for step, name in enumerate(("msm_15", "ragged", "msm_15", "unit_border", "ragged")):
            units = lay.layout(call, name)
            check(run(kz, s, call, units), units, "%s, step %d (%s)" % (call, step, name))
        assert neighbours() == before
    finally:
        s.free()


# ---- 8. two threads on one handle: the host form and the device form at once
@pytest.mark.parametrize("call", lay.CALLS)
def test_two_threads(kz, s12, call):
    a_units, b_units = lay.layout(call, "ragged"), lay.layout(call, "refused_at_border")
    serial_a = check(run(kz, s12, call, a_units), a_units, call + " ragged, serial")
    serial_b = check(run(kz, s12, call, b_units, device=True), b_units, call + " refused_at_border, serial")
    for turn in range(2):
        jobs = [Prepared(kz, s12, call, a_units), Prepared(kz, s12, call, b_units, device=True)]
        start = threading.Barrier(2)
        errors = []

        def work(job):
            try:
                start.wait(60)
                job.run()
            except Exception as e:                                 # noqa: BLE001
                errors.append(e)

        threads = [threading.Thread(target=work, args=(j,)) for j in jobs]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        what = "%s, two threads, turn %d" % (call, turn)
        check_equal(check(jobs[0].result(), a_units, what), serial_a, a_units, what + ", host form against serial")
        check_equal(check(jobs[1].result(), b_units, what), serial_b, b_units, what + ", device form against serial")


# ---- 9. kernel timing: the launch counts are the model's launch sets, and the bytes are the same with it on and off
@pytest.mark.parametrize("call", lay.CALLS)
def test_kernel_timing_counts_the_launch_sets(kz, setup_bytes, call):
    lib = kz.kzg.lib()
    s = _load(kz, setup_bytes, msm_bits=12)

    def launches(family):
        total, count = C.c_double(-1.0), C.c_long(-1)
        assert lib.kzg355_kernel_ms_stats(s.handle, family.encode(), C.byref(total), C.byref(count)) == 0
        assert (total.value > 0) == (count.value > 0)
        return count.value

    try:
        ragged, empty_first = lay.layout(call, "ragged"), lay.layout(call, "empty_chunk_first")
        lib.kzg355_reset_kernel_stats(s.handle)
        assert (launches(PER_CHUNK_FAMILY[call]), launches("cq_quotient")) == (0, 0)
        s.set_kernel_timing(True)
        timed = check(run(kz, s, call, ragged), ragged, call + " ragged, timing on")
        check(run(kz, s, call, empty_first), empty_first, call + " empty_chunk_first, timing on")
        chunks = lay.split(ragged) + lay.split(empty_first)
        counts = launches(PER_CHUNK_FAMILY[call]), launches("cq_quotient")
        assert counts == (len(chunks), sum(1 for c in chunks if c[2])) == (4, 3)
        # exactly CQ_CHUNK pairs, with riders behind them, are one launch set (only the count can tell: the bytes are right either way)
        full = lay.layout(call, "riders")[:12]
        assert lay.split(full) == [(0, 12, lay.CQ_CHUNK, lay.CQ_CHUNK)]
        check(run(kz, s, call, full), full, call + " one full chunk, timing on")
        counts = launches(PER_CHUNK_FAMILY[call]), launches("cq_quotient")
        assert counts == (5, 4)
        s.set_kernel_timing(False)
        check_equal(check(run(kz, s, call, ragged), ragged, call + " ragged, timing off"), timed, ragged, call + ", timing off against on")
        assert (launches(PER_CHUNK_FAMILY[call]), launches("cq_quotient")) == counts
    finally:
        s.free()
