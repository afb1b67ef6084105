"""The replay set on the GPU (``mastic_amd.NonceSet``, ``mastic_nonce_set_*``):
admitting a batch marks a nonce fresh iff the set did not hold it and it does
not occur earlier in the batch, whatever the hash key, the table size or the
scheduling.  Every expected mask comes from the model below (a ``dict`` walked
in index order), never from the code under test.

Sizes 0, 1, 63, 64, 65, 257 and 4099 are the wave and workgroup edges (64 lanes,
256 per workgroup); 4099 nonces are 17 workgroups, so duplicates half a batch
apart are inserted by workgroups on different XCDs."""
import random

import numpy as np
import pytest

from conftest import PKG_ROOT  # noqa: F401

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 63, 64, 65, 257, 4099]


class Model:
    def __init__(self):
        self.seen = {}

    def admit(self, nonces):
        fresh = []
        for x in nonces:
            fresh.append(0 if x in self.seen else 1)
            self.seen[x] = True
        return fresh


def _nonces(seed, n):
    rng = random.Random(seed)
    return [rng.randbytes(16) for _ in range(n)]


@pytest.fixture(scope="module")
def mastic(gpu_available):
    import mastic_amd
    return mastic_amd.MasticCount(8)


def _resident(mastic, nonces):
    from mastic_amd.vdaf import Reports
    rep = Reports(mastic, len(nonces))
    rep.upload(b"".join(nonces), None)
    return rep


def _check_admit(ns, model, nonces, resident=None):
    want = model.admit(nonces)
    got = ns.admit(resident if resident is not None else b"".join(nonces))
    assert got.dtype == np.uint8 and got.tolist() == want
    assert len(ns) == len(model.seen)


@pytest.mark.parametrize("n", SIZES)
def test_all_distinct_then_all_replayed(mastic, n):
    from mastic_amd import NonceSet
    ns, model = NonceSet(mastic), Model()
    x = _nonces(100 + n, n)
    _check_admit(ns, model, x)
    assert len(ns) == n
    _check_admit(ns, model, x)  # every one a replay of the set now
    assert len(ns) == n and ns.contains(b"".join(x)).tolist() == [1] * n


@pytest.mark.parametrize("n", SIZES[1:])
def test_all_equal_lowest_index_wins(mastic, n):
    """Every lane contends for one slot; the mask must be [1, 0, 0, ...]."""
    from mastic_amd import NonceSet
    ns = NonceSet(mastic)
    x = _nonces(200 + n, 1) * n
    assert ns.admit(_resident(mastic, x)).tolist() == [1] + [0] * (n - 1)
    assert len(ns) == 1


@pytest.mark.parametrize("n", SIZES[1:])
def test_pairs_adjacent_and_half_a_batch_apart(mastic, n):
    from mastic_amd import NonceSet
    half = n // 2
    x = _nonces(300 + n, half + 1)
    adjacent = [x[i // 2] for i in range(2 * half)] + [x[half]] * (n - 2 * half)
    apart = x[:half] + x[:half] + [x[half]] * (n - 2 * half)
    for batch in (adjacent, apart):
        assert len(batch) == n
        ns, model = NonceSet(mastic), Model()
        _check_admit(ns, model, batch, _resident(mastic, batch))
        assert len(ns) == len(set(batch))


@pytest.mark.parametrize("n", [65, 4099])
def test_nonces_differing_in_one_word(mastic, n):
    """Keys equal in three of their four words are different keys, for each word."""
    from mastic_amd import NonceSet
    ns, model = NonceSet(mastic), Model()
    base = _nonces(400 + n, 1)[0]
    for w in range(4):
        batch = []
        for i in range(n):
            word = (int.from_bytes(base[4 * w:4 * w + 4], "little") ^ ((i % (n - 3)) + 1)).to_bytes(4, "little")
            batch.append(base[:4 * w] + word + base[4 * w + 4:])  # the last 3 repeat the first 3
        _check_admit(ns, model, batch)
    assert len(ns) == 4 * (n - 3)
    assert ns.contains(base).tolist() == [0]


@pytest.mark.parametrize("n", SIZES[1:])
def test_mixed_replay_and_contains(mastic, n):
    from mastic_amd import NonceSet
    rng = random.Random(500 + n)
    ns, model = NonceSet(mastic), Model()
    a, new, never = _nonces(510 + n, n), _nonces(520 + n, n), _nonces(530 + n, n)
    _check_admit(ns, model, a)
    mix = a + new + rng.choices(new, k=n // 2)
    rng.shuffle(mix)
    _check_admit(ns, model, mix, _resident(mastic, mix))
    assert len(ns) == 2 * n
    q = a + new + never
    assert ns.contains(b"".join(q)).tolist() == [1] * (2 * n) + [0] * n
    assert len(ns) == 2 * n  # a query inserts nothing


def test_growth_from_a_hint_of_one(mastic):
    from mastic_amd import NonceSet
    ns, model = NonceSet(mastic, capacity=1), Model()
    everything = []
    for (k, n) in enumerate([1, 63, 65, 257, 4099]):
        batch = _nonces(600 + k, n) + everything[:n // 3]  # new ones and replays of what the set holds
        _check_admit(ns, model, batch)
        everything += batch[:n]
        assert len(ns) == len(everything)
        never = _nonces(650 + k, 50)
        assert ns.contains(b"".join(everything + never)).tolist() == [1] * len(everything) + [0] * 50


def test_input_paths_views_and_keys_agree(mastic):
    from mastic_amd import NonceSet
    x = _nonces(700, 100)
    x[40] = x[7]    # a duplicate inside the view below
    x[90] = x[2]    # one whose first copy lies outside it
    rep = _resident(mastic, x)
    want = Model().admit(x)
    masks = [NonceSet(mastic).admit(b"".join(x)).tolist(), NonceSet(mastic).admit(rep).tolist(),
             NonceSet(mastic, hash_key=bytes(16)).admit(rep).tolist(),
             NonceSet(mastic, hash_key=bytes(range(1, 17))).admit(rep).tolist()]
    assert masks == [want] * 4
    # a view admits its own rows only
    ns = NonceSet(mastic)
    view = rep.view(5, 70)
    assert ns.admit(view).tolist() == Model().admit(x[5:75])
    assert len(ns) == len(set(x[5:75])) == 69
    assert ns.contains(b"".join(x)).tolist() == [1 if v in set(x[5:75]) else 0 for v in x]
    # reports of another ctx are refused
    import mastic_amd
    other = mastic_amd.MasticCount(8)
    with pytest.raises(ValueError):
        ns.admit(_resident(other, x[:4]))
    assert len(ns) == 69


def test_checkpoint_round_trip(mastic):
    from mastic_amd import NonceSet
    ns = NonceSet(mastic)
    x = _nonces(800, 3000)
    ns.admit(b"".join(x + x[:100]))
    data = ns.export()
    assert len(data) == 16 * 3000
    assert sorted(data[i:i + 16] for i in range(0, len(data), 16)) == sorted(x)
    restored = NonceSet(mastic, capacity=3000)
    assert restored.load(data) == 3000 and len(restored) == 3000
    never = _nonces(801, 10)
    assert restored.contains(b"".join(x + never)).tolist() == [1] * 3000 + [0] * 10
    assert restored.admit(b"".join(x[:5] + never[:2])).tolist() == [0] * 5 + [1] * 2
    assert NonceSet(mastic).export() == b""


def test_allocation_failure_leaves_the_set_unchanged(mastic):
    from mastic_amd import MasticError, NonceSet
    ns, model = NonceSet(mastic), Model()
    a = _nonces(900, 300)
    _check_admit(ns, model, a)
    grow = _nonces(901, 4099) + a[:10]  # past the minimum table: the admit must grow it
    resident = _resident(mastic, grow)
    q = b"".join(a + grow[:50])
    before = ns.contains(q).tolist()
    mastic.set_test_hooks(fail_allocs=1)  # the new table's allocation
    with pytest.raises(MasticError) as e:
        ns.admit(resident)
    assert e.value.code == -12
    assert mastic.set_test_hooks() == 0, "the injected allocation failure was not reached"
    assert len(ns) == 300 and ns.contains(q).tolist() == before == [1] * 300 + [0] * 50
    _check_admit(ns, model, grow, resident)  # the same call then succeeds
    assert len(ns) == 300 + 4099
    # host nonces: the staging buffer's allocation fails the same way
    more = _nonces(902, 9000)
    mastic.set_test_hooks(fail_allocs=1)
    with pytest.raises(MasticError) as e:
        ns.admit(b"".join(more))
    assert e.value.code == -12 and mastic.set_test_hooks() == 0
    assert len(ns) == 300 + 4099 and ns.contains(b"".join(more[:20])).tolist() == [0] * 20
    _check_admit(ns, model, more)
    assert ns.contains(q).tolist() == [1] * 350
