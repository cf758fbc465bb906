#include "slot_plan.h"

#include <ostream>
#include <set>

namespace bammhost {

SlotPlan make_slot_plan(size_t n_slots, size_t cv_fold, bool em, bool fdr, bool one_slot_chain, const std::vector<int>& device_list) {
    SlotPlan p;
    const size_t cvF = std::max<size_t>(1, cv_fold);
    p.n_slots = n_slots; p.em = em; p.fdr = fdr;
    p.overlap = fdr && em && n_slots >= cvF + 1;
    p.fold_slot.assign(cvF, 0);
    for (size_t d = 0; d < (p.overlap ? n_slots - cvF : n_slots); d++) p.em_slots.push_back(d);
    for (size_t f = 0; f < cvF; f++) p.fold_slot[f] = p.overlap ? n_slots - cvF + f : f % n_slots;
    if (one_slot_chain) p.em_slots.resize(1);
    std::set<int> em_devices;
    for (size_t d : p.em_slots) em_devices.insert(device_list[d]);
    p.distinct = em_devices.size() == p.em_slots.size();
    p.sharded = p.em_slots.size() > 1 && em;
    return p;
}

void print_slot_plan(std::ostream& os, const SlotPlan& p, const std::vector<int>& device_list, bool score) {
    os << "  plan over " << p.n_slots << " GPU slot(s) [devices";
    for (int dv : device_list) os << ' ' << dv;
    os << "]:";
    if (p.em) os << " main EM on slot(s) 0.." << p.em_slots.size() - 1 << (p.sharded ? (p.distinct ? " (sharded, RCCL all-reduce per iteration)" : " (sharded, host-staged all-reduce: a device is listed twice)") : "");
    if (p.fdr) {
        os << "; fold -> slot";
        for (size_t f = 0; f < p.fold_slot.size(); f++) os << ' ' << f << "->" << p.fold_slot[f];
        os << (p.overlap ? " (while the main run trains)" : " (after the main run)");
    }
    if (score) os << "; --scoreSeqset on slot 0";
    os << std::endl;
}

}  // namespace bammhost
