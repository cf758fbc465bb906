// The plan: which GPU slot does what (FDR.cpp:37-127, mainBaMM.cpp:131-147).  A pure function of the command
// line -- no HIP, no globals -- shared by the BaMMmotif driver and the test hooks (bh_slot_plan).
//   * the main EM run is sharded over its group of slots, one all-reduce of the count table per iteration: RCCL when
//     the group's devices are distinct, else (a device listed twice: self-tests on a 1-GPU box) the host-staged sum;
//   * --FDR trains fold f on fold_slot[f] from the SEED model, so the folds do not wait for the main run: with at
//     least cvFold + 1 slots the folds take the last cvFold of them and the main run the others, AT THE SAME TIME
//     (8 GPUs, 5 folds: 3 + 5, no idle device); with fewer slots the main run uses all of them first and the folds
//     then go round them (fold f on slot f mod N).
//   --advanceEM --optimizeQ re-estimates q after every sequence (EM.cpp:321): that chain runs on one slot.
#pragma once
#include <algorithm>
#include <cstddef>
#include <iosfwd>
#include <vector>

namespace bammhost {

struct SlotPlan {
    size_t n_slots = 1;
    bool em = false, fdr = false;
    std::vector<size_t> em_slots;          // the main run's group: slots 0 .. em_slots.size() - 1
    std::vector<size_t> fold_slot;         // [max(1, cvFold)]
    bool overlap = false;                  // the folds train while the main run does, on slots of their own
    bool sharded = false;                  // the main run spans more than one slot
    bool distinct = true;                  // no device twice in the main run's group
    bool in_em_group(size_t d) const { return d < em_slots.size(); }
    bool runs_folds(size_t d) const { return fdr && std::find(fold_slot.begin(), fold_slot.end(), d) != fold_slot.end(); }
};

// one_slot_chain: --advanceEM --optimizeQ; device_list: the device of every slot (n_slots entries at least)
SlotPlan make_slot_plan(size_t n_slots, size_t cv_fold, bool em, bool fdr, bool one_slot_chain, const std::vector<int>& device_list);
// the plan line of --timing
void print_slot_plan(std::ostream& os, const SlotPlan& plan, const std::vector<int>& device_list, bool score);

}  // namespace bammhost
