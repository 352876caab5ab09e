// mcs_dtrade_grant.h — arguments of the external traders' kernels (mcs_dtrade_grant.hip; host side in
// mcs_dtrade.cpp, DESIGN.md §14 "External traders").  The host stably groups a call's entries by the
// cluster they act on (a provide call: the responder; a receive call: the receiving cluster) and
// uploads the grouped entries with the groups' ranges: one wave per group, entries in array order.
#pragma once
#include "mcs_dtrade_internal.h"

namespace mcs {

struct DtGrantGroup {
    uint32_t cluster, begin, end, pad;  // grouped entries [begin, end) act on local cluster `cluster`
};

struct DtGrantStatus {  // zeroed by the call's upload, read back with its results
    uint32_t flags;     // MCS_FLAG_OVERFLOW / MCS_FLAG_VNODE_OVERFLOW: escalate and replay; LOG_OVERFLOW
    uint32_t added;     // Foreign records of the call
    unsigned long long n_foreign;  // the log's counter after the call
};

struct DtGrantArgs {
    const mcs_vnode_request* req;  // provide: the grouped requests
    const mcs_vnode_grant* node;   // receive: the grouped nodes
    const uint32_t* order;         // grouped place -> place in the caller's array
    const uint32_t* inv;           // place in the caller's array -> grouped place
    const uint32_t* soff;          // grouped place -> first row of the request's stash
    const DtGrantGroup* groups;
    mcs_vnode_result* res;         // in the caller's order
    uint32_t* cnt;                 // rows visited, in the caller's order
    unsigned long long* stash;     // {uint(coreDiff), uint(memDiff)} per visited row
    DtGrantStatus* status;
    unsigned long long n_foreign;  // the log's counter before the call
    uint32_t n, n_groups, T, pad;
};

// the walk and the log: two launches whatever n is
hipError_t launch_dtrade_grant_provide(const DtArgs& a, const DtGrantArgs& g, hipStream_t s);
hipError_t launch_dtrade_grant_receive(const DtArgs& a, const DtGrantArgs& g, hipStream_t s);

}  // namespace mcs
