"""The CLI's GPU slot plan (host/slot_plan.cpp: which slot trains the main run, which runs which fold, whether the main run
is sharded and over what kind of all-reduce) through its hook in libbamm_host.so.  The expected plans below are written out
by hand from the rule stated in host/slot_plan.h:

  * --FDR with --EM and at least cvFold + 1 slots: the folds take the LAST cvFold slots (fold f on slot N - cvFold + f) and
    the main run the others, at the same time (overlap);
  * otherwise the main run uses all N slots and fold f goes on slot f mod N;
  * --advanceEM --optimizeQ: the main run is a chain on one slot;
  * sharded = --EM on more than one slot; distinct = no device twice among the main run's slots."""
import ctypes as C

import numpy as np
import pytest

from bammmotif2_amd import build


@pytest.fixture(scope="module")
def host():
    build.build_host()
    return C.CDLL(build.HOST_LIB)


def plan(host, n_slots, cv_fold, em=True, fdr=True, chain=False, devices=None):
    devices = np.asarray(list(range(n_slots)) if devices is None else devices, np.int32)
    assert len(devices) == n_slots
    em_slots = np.full(n_slots, 99, np.uint64)
    fold_slot = np.full(max(1, cv_fold), 99, np.uint64)
    in_em, folds_on = np.full(n_slots, 9, np.uint8), np.full(n_slots, 9, np.uint8)
    n_em = C.c_uint64(99)
    overlap, sharded, distinct = C.c_int(9), C.c_int(9), C.c_int(9)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = host.bh_slot_plan(C.c_uint64(n_slots), C.c_uint64(cv_fold), int(em), int(fdr), int(chain), p(devices), C.byref(n_em), p(em_slots),
                           p(fold_slot), C.byref(overlap), C.byref(sharded), C.byref(distinct), p(in_em), p(folds_on))
    assert rc == 0
    return {"em_slots": em_slots[:n_em.value].tolist(), "fold_slot": fold_slot.tolist(), "overlap": bool(overlap.value),
            "sharded": bool(sharded.value), "distinct": bool(distinct.value), "in_em_group": in_em.astype(bool).tolist(),
            "runs_folds": folds_on.astype(bool).tolist()}


def expect(em_slots, fold_slot, overlap, sharded, n_slots, distinct=True, fdr=True):
    return {"em_slots": em_slots, "fold_slot": fold_slot, "overlap": overlap, "sharded": sharded, "distinct": distinct,
            "in_em_group": [d in em_slots for d in range(n_slots)],
            "runs_folds": [fdr and d in fold_slot for d in range(n_slots)]}


@pytest.mark.parametrize("n_slots, cv_fold, want", [
    # fewer than cvFold + 1 slots: the main run on all of them, then fold f on slot f mod N
    (1, 4, expect([0], [0, 0, 0, 0], False, False, 1)),
    (2, 4, expect([0, 1], [0, 1, 0, 1], False, True, 2)),
    (4, 4, expect([0, 1, 2, 3], [0, 1, 2, 3], False, True, 4)),
    # overlap: the folds on the last cvFold slots, the main run on the first N - cvFold
    (5, 4, expect([0], [1, 2, 3, 4], True, False, 5)),
    (8, 5, expect([0, 1, 2], [3, 4, 5, 6, 7], True, True, 8)),
    (6, 5, expect([0], [1, 2, 3, 4, 5], True, False, 6)),           # a main run of one slot is not sharded
])
def test_folds_and_main_run_share_the_slots_as_the_rule_says(host, n_slots, cv_fold, want):
    assert plan(host, n_slots, cv_fold) == want


def test_the_chain_of_advanceEM_optimizeQ_runs_on_one_slot(host):
    # with --FDR (4 folds): overlap, the folds on slots 4..7; of the main run's slots 0..3 only slot 0 is left
    assert plan(host, 8, 4, chain=True) == expect([0], [4, 5, 6, 7], True, False, 8)
    # --EM alone: all 8 slots would shard the run; the chain keeps slot 0
    assert plan(host, 8, 4, fdr=False, chain=True) == expect([0], [0, 1, 2, 3], False, False, 8, fdr=False)
    assert plan(host, 8, 4, fdr=False) == expect(list(range(8)), [0, 1, 2, 3], False, True, 8, fdr=False)


def test_a_device_listed_twice_is_not_distinct(host):
    assert plan(host, 3, 4, devices=[0, 0, 1]) == expect([0, 1, 2], [0, 1, 2, 0], False, True, 3, distinct=False)
    assert plan(host, 3, 4, devices=[0, 2, 1]) == expect([0, 1, 2], [0, 1, 2, 0], False, True, 3, distinct=True)
    # the main run's group decides: 0,1 train (distinct), the folds on 1,1,2,2 may share a device
    assert plan(host, 6, 4, devices=[0, 1, 1, 1, 2, 2]) == expect([0, 1], [2, 3, 4, 5], True, True, 6, distinct=True)


def test_fdr_without_em_goes_round_all_slots_and_never_overlaps(host):
    assert plan(host, 8, 4, em=False) == expect(list(range(8)), [0, 1, 2, 3], False, False, 8)
    assert plan(host, 8, 10, em=False) == expect(list(range(8)), [0, 1, 2, 3, 4, 5, 6, 7, 0, 1], False, False, 8)
