"""GPU parity for the resident 512^3 kernels whose look-ahead request is held in place against the compiler (ca_resident_kernel.inc:
resident_pair_run, resident_run): where a tile asks for its neighbours' faces changes when an answer arrives, never what is computed.
Batches of 8, 9 and 21 steps — the even and the odd tail of the step loop unrolled by two, and the shortest batch the resident path
takes (resident_min = 8) — for a rule compiled at run time and for the pre-built start-up rule; the final state AND the other
ping-pong buffer bit for bit against the oracle."""
import numpy as np
import pytest

import oracle_lib as ol
from cellularautomatons3d_amd import host, slab
from gpu_common import rules, set_rules

pytestmark = pytest.mark.gpu

G = 512
SEED = 0xCA3D0001
BATCHES = (8, 9, 21)


@pytest.fixture(scope="module")
def eng():
    from cellularautomatons3d_amd import Engine

    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def start_state():
    st = host.random_fill(host.words_per_buffer(G), seed=SEED)
    st.setflags(write=False)
    return st


_ORACLE = {}


def _oracle_states(tables, st):
    """The oracle's states in front of and behind every batch boundary, computed once per rule and shared by the forms."""
    if tables not in _ORACLE:
        r = rules(tables)
        states, cur, total = {0: st}, st, 0
        for n in BATCHES:
            prev = ol.packed_run(G, cur, r, n - 1)
            cur = ol.packed_step(G, prev, r)
            total += n
            states[total - 1], states[total] = prev, cur
        for v in states.values():
            v.setflags(write=False)
        _ORACLE[tables] = states
    return _ORACLE[tables]


@pytest.mark.parametrize("tables,form", [("vn_b24_s135", "pair"), ("default", "pair"), ("default", 32), ("default", 16)])
def test_resident_512_batches_match_the_oracle(eng, start_state, tables, form):
    r = rules(tables)
    pair = form == "pair"
    eng.configure(G)
    eng.set_option("resident_pair", int(pair))
    eng.set_option("resident_rows", 32 if pair else form)
    eng.set_option("resident_zsplit", 1)
    set_rules(eng, r)
    try:
        assert eng.info().kernel_name == (b"ca_resident_vn" if tables == "default" else b"ca_resident_vn(jit)"), eng.info().kernel_name
        want = _oracle_states(tables, start_state)
        eng.upload_state(start_state)
        total = 0
        for n in BATCHES:
            eng.step(n)
            total += n
            assert eng.info().step == total and eng.info().current_buffer == total % 2
            np.testing.assert_array_equal(eng.read_state(), want[total], err_msg=f"{tables} {form}: after a batch of {n}")
            other = slab.device_tensor(*eng.device_buffer(1 - total % 2), 0).cpu().numpy().view(np.uint32)
            np.testing.assert_array_equal(other, want[total - 1], err_msg=f"{tables} {form}: the other buffer after a batch of {n}")
    finally:
        eng.set_option("resident_pair", 1)
        eng.set_option("resident_rows", 32)
