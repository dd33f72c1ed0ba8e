"""-m gpu: what the five batch entry points share around their launches - the device table of the members' records, the join and
the fork of the members' streams - through psm_compute_batch (float and 8-bit volumes), psm_sgm_compute_batch,
psm_sgm_select_maps_batch, psm_joint_wmf_batch and psm_score_batch.  Every comparison is bit-equality (np.array_equal, ==) with
the same call made singly on a twin context holding the same inputs: there is no tolerance anywhere in this file.  Every member of
every call holds an input of its own, and members are replaced between calls, so a table that was not refreshed, a slot that was
rewritten too early or a stream that was not waited for leaves some member with the result of another input."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_INPUTS = 7            # distinct inputs per entry point; a call has at most 4 members, so the members of a call never share one


@pytest.fixture(scope="module")
def psm():
    from primestereomatch_amd import capi
    capi.load()
    assert capi.device_count() >= 1, "no HIP device visible"
    import primestereomatch_amd as P
    return P


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


class Compute:
    """psm_compute_batch against CostConst_GPU + CostFilter_GPU + DispSelect_GPU; a new pair is staged and adopted by the batch."""
    W, H, D = 67, 45, 16

    def __init__(self, dtype):
        self.dtype = dtype

    @functools.lru_cache(maxsize=None)
    def inputs(self, k):
        from primestereomatch_amd import synth
        return frozen(*synth.make_pair(self.W, self.H, self.D, seed=40 + k)[:2])

    def open(self, P, k):
        return P.DispEst(*self.inputs(k), self.D, dtype=self.dtype)

    def load(self, de, k):
        de.setInputImages_async(*self.inputs(k))

    def rearm(self, de, k):
        pass

    def run(self, des):
        from primestereomatch_amd import dispest
        dispest.compute_batch(des)
        return [tuple(m.copy() for m in de.download_maps()) for de in des]

    def single(self, de):
        de.CostConst_GPU(); de.CostFilter_GPU(); de.DispSelect_GPU()
        return de.lDisMap.copy(), de.rDisMap.copy()


class Sgm(Compute):
    """psm_sgm_compute_batch against SGBM_GPU; a new pair is staged and adopted on the member's own stream."""

    def __init__(self):
        super().__init__("f32")

    def load(self, de, k):
        de.setInputImages_async(*self.inputs(k))
        de.CostConst_GPU()

    def results(self, de):
        return (de.sgm_disparity().copy(),) + tuple(a.copy() for a in de.sgm_costs())

    def run(self, des):
        from primestereomatch_amd import dispest
        dispest.sgbm_batch(des)
        return [self.results(de) for de in des]

    def single(self, de):
        de.SGBM_GPU()
        return self.results(de)


class SgmMaps(Sgm):
    """psm_sgm_select_maps_batch against SGBMSelect_GPU; the S it reads comes from the member's own SGBM_GPU."""

    def load(self, de, k):
        super().load(de, k)
        de.SGBM_GPU()

    def rearm(self, de, k):
        de.SGBM_GPU()

    def run(self, des):
        from primestereomatch_amd import dispest
        dispest.sgbm_select_batch(des)
        return [tuple(m.copy() for m in de.download_maps()) for de in des]

    def single(self, de):
        de.SGBM_GPU()
        return tuple(m.copy() for m in de.SGBMSelect_GPU())


class JointWmf:
    """psm_joint_wmf_batch against JointWMF_GPU: both maps and both clusterings; a new pair is staged and adopted on the member's
    own stream, its maps are uploaded behind it."""
    W, H, D, RADIUS, CLUSTERS = 33, 17, 8, 4, 4

    @functools.lru_cache(maxsize=None)
    def inputs(self, k):
        g = np.random.default_rng(3000 + k)
        return frozen(g.integers(0, 256, (self.H, self.W, 3), dtype=np.uint8), g.integers(0, 256, (self.H, self.W, 3), dtype=np.uint8),
                      g.integers(0, 256, (2, self.H, self.W), dtype=np.uint8))

    def open(self, P, k):
        l, r, maps = self.inputs(k)
        de = P.DispEst(l, r, self.D)
        de.upload_maps(*maps)
        return de

    def load(self, de, k):
        l, r, maps = self.inputs(k)
        de.setInputImages_async(l, r)
        de.CostConst_GPU()
        de.upload_maps(*maps)

    def rearm(self, de, k):
        de.upload_maps(*self.inputs(k)[2])          # (the filter rewrote them in place)

    def results(self, de):
        out = [de.lDisMap.copy(), de.rDisMap.copy()]
        for side in (0, 1):
            out.extend(de.jwmf_clusters(side))
        return tuple(out)

    def run(self, des):
        from primestereomatch_amd import dispest
        dispest.joint_wmf_batch(des, self.RADIUS, 0.0, self.CLUSTERS, 0)
        return [self.results(de) for de in des]

    def single(self, de):
        de.JointWMF_GPU(self.RADIUS, 0.0, self.CLUSTERS, 0)
        return self.results(de)


class Score:
    """psm_score_batch against Score_GPU: the record and the three planes; new maps and a new truth are uploaded."""
    W, H, D = 130, 9, 16

    @functools.lru_cache(maxsize=None)
    def inputs(self, k):
        g = np.random.default_rng(4000 + k)
        plane = lambda: g.integers(0, 256, (self.H, self.W)).astype(np.uint8)
        return frozen(plane(), plane(), plane(), g.choice(np.array([0, 1, 127, 128, 254, 255], np.uint8), (self.H, self.W)))

    def open(self, P, k):
        z = np.zeros((self.H, self.W, 3), np.uint8)
        de = P.DispEst(z, z, self.D)
        de.set_score_params(3, 1)
        self.load(de, k)
        return de

    def load(self, de, k):
        lmap, rmap, gt, mask = self.inputs(k)
        de.set_truth(gt, mask)
        de.upload_maps(lmap, rmap)

    def rearm(self, de, k):
        pass

    def run(self, des):
        from primestereomatch_amd import dispest
        recs = dispest.score_batch(des)
        return [(rec,) + tuple(p.copy() for p in de.score_maps(right=True)) for de, rec in zip(des, recs)]

    def single(self, de):
        rec = de.Score_GPU()
        return (rec,) + tuple(p.copy() for p in de.score_maps(right=True))


ENTRIES = {"compute-f32": Compute("f32"), "compute-u8": Compute("u8"), "sgm": Sgm(), "sgm-maps": SgmMaps(), "joint-wmf": JointWmf(),
           "score": Score()}
KINDS = sorted(ENTRIES)


@functools.lru_cache(maxsize=None)
def expected(kind, k):
    """The single call on a twin context that holds input k: computed once, shared by every test of the entry point."""
    import primestereomatch_amd as P
    e = ENTRIES[kind]
    with e.open(P, k) as twin:
        return e.single(twin)


def same(a, b):
    return np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b


class Rig:
    """A pool of contexts of one entry point.  call(members): every member gets an input it does not hold yet (fresh) or is made
    ready for the same call again, the batch runs with members[0] as its head, and every member's result is compared."""

    def __init__(self, P, kind, n, shared=False):
        self.kind, self.e = kind, ENTRIES[kind]
        self.k = list(range(n))
        self.des = [self.e.open(P, k) for k in self.k]
        self.tick = n
        if shared:
            from primestereomatch_amd import dispest
            dispest.share_streams(self.des)

    def close(self):
        for de in self.des:
            de.close()

    def call(self, members, fresh=True):
        taken = set()
        for i in members:
            if fresh:
                while self.tick % N_INPUTS in taken | {self.k[i]}:      # (not the one it holds, not another member's of this call)
                    self.tick += 1
                self.k[i] = self.tick % N_INPUTS
                self.e.load(self.des[i], self.k[i])
            else:
                self.e.rearm(self.des[i], self.k[i])
            taken.add(self.k[i])
        got = self.e.run([self.des[i] for i in members])
        assert len(taken) == len(members)
        for i, g in zip(members, got):
            want = expected(self.kind, self.k[i])
            bad = [j for j, (a, b) in enumerate(zip(g, want)) if not same(a, b)]
            print(f"[batch-tables] {self.kind} members {members}: context {i} input {self.k[i]}: differing results {bad}")
            assert len(g) == len(want) and not bad, (members, i, bad)


@pytest.fixture
def rig(psm):
    rigs = []

    def make(kind, n, shared=False):
        rigs.append(Rig(psm, kind, n, shared))
        return rigs[-1]

    yield make
    for r in rigs:
        r.close()


@pytest.mark.parametrize("kind", KINDS)
def test_grow_shrink_repeat_on_one_head(rig, kind):
    """Batches of 2, 4, 1, 3, 3 members behind the same head: the table grows, is used partly, and the last call repeats the one
    before it verbatim - nothing to upload, and the result is still right."""
    r = rig(kind, 5)
    r.call([0, 1])
    r.call([0, 2, 3, 4])
    r.call([0])
    r.call([0, 4, 1])
    r.call([0, 4, 1], fresh=False)


@pytest.mark.parametrize("shared", (False, True), ids=("own-streams", "shared-streams"))
@pytest.mark.parametrize("kind", KINDS)
def test_both_slots_reused(rig, kind, shared):
    """Five consecutive calls with changed records - new inputs (the image slots of compute and SGM alternate) and other members:
    both page-locked slots are refilled, behind copies that may not have executed."""
    r = rig(kind, 5, shared)
    for members in ([0, 1, 2], [0, 3, 1], [0, 2, 4], [0, 4, 3], [0, 1, 2]):
        r.call(members)


@pytest.mark.parametrize("kind", KINDS)
def test_head_and_member_change_roles(rig, kind):
    r = rig(kind, 2)
    r.call([0, 1])
    r.call([1, 0])
    r.call([0, 1])


@pytest.mark.parametrize("kind", KINDS)
def test_release_scratch_between_two_batches(rig, kind):
    """psm_release_scratch on the head gives the SGM and score tables back with their stages' buffers; psm_compute_batch's and
    JointWMF's stay.  The same members, the same inputs: the second batch is right either way."""
    r = rig(kind, 3)
    r.call([0, 1, 2])
    r.des[0].release_scratch()
    r.call([0, 1, 2], fresh=False)
