// mcs_dtrade_grant.hip — gfx950 kernels of the external traders' calls on a trading session
// (DESIGN.md §14 "External traders"): mcs_trade_session_provide_vnodes (ProvideVirtualNode ->
// AllocateVirtualNodeResources, cluster.go:87-125) and mcs_trade_session_receive_vnodes
// (ReceiveVirtualNode -> AddVirtualNode, cluster.go:65-85), in batches, between two slices, on the
// live lock-step state the last executed tick left in HBM.
//
//   dt_grant_walk_kernel  one wave per distinct responder of the call; the wave walks its responder's
//                         requests in array order.  Rows come in 64 at a time, one u64 per lane; the
//                         serial recurrence over the rows runs on readlane broadcasts and leaves at the
//                         first row with both halves 0; lane i keeps the diffs of row i.  The visited rows
//                         are a prefix, so the commits are lane-parallel: the j-th visited row takes the
//                         j-th free running slot (ballot over sfin + mbcnt ranks).  The diffs are stashed
//                         per request for the log.
//   dt_grant_log_kernel   after the kernel boundary: the exclusive scan of the visit counts over the
//                         call's requests in array order, then the Foreign records, coalesced; the log's
//                         counter in the control block.
//   dt_grant_recv_kernel  one wave per distinct receiving cluster: its new rows, lane-parallel.
// No wave reads what another wave of the same launch wrote: the hand-over between the walk and the log
// is the kernel boundary.  A wave re-reads rows it committed itself (the second request to a responder
// sees the first): those stores and loads are agent-scope atomics (L2), never this CU's vector L1.
#include "mcs_dtrade_dev.h"
#include "mcs_dtrade_grant.h"

namespace mcs {
namespace {

__device__ __forceinline__ uint32_t lane_rank(const unsigned long long mask) {
    return (uint32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

__global__ __launch_bounds__(64) void dt_grant_walk_kernel(DtArgs a, DtGrantArgs g) {
    const uint32_t grp = blockIdx.x, lane = threadIdx.x;
    if (grp >= g.n_groups) return;
    const DtGrantGroup gr = g.groups[grp];
    const uint32_t r = gr.cluster;  // (host-checked: r < C)
    const uint32_t n0 = a.node_off[r], N = a.node_off[r + 1] - n0;
    DtCluster* cl = &a.cl[r];
    uint32_t nv = cl->nv;
    nv = nv < a.V ? nv : a.V;
    const uint32_t NN = N + nv, S = a.S, T = g.T;
    const size_t rsb = (size_t)r * S;
    unsigned long long* const tn = a.tn + n0;
    unsigned long long* const vn = a.vn + (size_t)r * a.V;
    uint32_t taken = 0, minf = kEmpty;  // running slots this wave took, their earliest finish
    uint32_t cursor = 0;                // every slot below it is taken (none is released in here)
    bool ovf = false;
    for (uint32_t i = gr.begin; i < gr.end && !ovf; ++i) {
        const mcs_vnode_request q = g.req[i];
        const uint32_t orig = g.order[i];
        unsigned long long* const stash = g.stash + 2ull * g.soff[i];
        uint32_t rc = q.cores, rm = q.memory, k = 0;
        const uint32_t fin = T + q.time_s;  // (host-checked: no wrap)
        for (uint32_t b = 0; b < NN; b += kWave) {
            if (rc == 0u && rm == 0u) break;  // cluster.go:90-92
            const uint32_t row = b + lane, rw = row < NN ? row : NN - 1u;
            unsigned long long* const np_ = rw < N ? &tn[rw] : &vn[rw - N];
            const unsigned long long v = ld64(np_);
            const uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
            const uint32_t jn = NN - b < (uint32_t)kWave ? NN - b : (uint32_t)kWave;
            unsigned long long myc = 0ull, mym = 0ull;
            uint32_t kb = 0;
            // the recurrence over the block's rows on broadcast values; lane j keeps row j's diffs
            for (uint32_t j = 0; j < jn; ++j) {
                if (rc == 0u && rm == 0u) break;
                const unsigned long long vj = (unsigned long long)readlane(lo, j) | ((unsigned long long)readlane(hi, j) << 32);
                unsigned long long fc, fm;
                dt_vnode_visit(vj, rc, rm, fc, fm);
                myc = lane == j ? fc : myc;
                mym = lane == j ? fm : mym;
                ++kb;
            }
            const bool vis = lane < kb;
            if (vis) {
                stash[2u * row] = myc;
                stash[2u * row + 1u] = mym;
            }
            k += kb;
            if (q.time_s == 0u) continue;  // RunJob sleeps 0: logged, holds nothing, takes no slot
            // go node.RunJob(Foreign) (cluster.go:116): the row's counter now, a running slot until fin
            if (vis) {
                const unsigned long long nv_ = (unsigned long long)(lo - (uint32_t)myc) |
                                               ((unsigned long long)(hi - (uint32_t)mym) << 32);
                __hip_atomic_store(np_, nv_, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            uint32_t got = 0;
            for (uint32_t sb = cursor; sb < S; sb += kWave) {
                const uint32_t s = sb + lane;
                const bool fr = s < S && ld32(&a.sfin[rsb + s]) == kEmpty;
                const unsigned long long fmask = __ballot(fr);
                const uint32_t rank = got + lane_rank(fmask);
                // (every lane takes part in the exchange: the slot's lane reads the row's lane)
                const uint32_t src = rank < kb ? rank : 0u;
                const uint32_t sc_ = (uint32_t)__shfl((int)(uint32_t)myc, (int)src);
                const uint32_t sm_ = (uint32_t)__shfl((int)(uint32_t)mym, (int)src);
                if (fr && rank < kb) {
                    __hip_atomic_store(&a.sfin[rsb + s], fin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    a.snode[rsb + s] = b + rank;
                    a.scm[rsb + s] = (unsigned long long)sc_ | ((unsigned long long)sm_ << 32);
                }
                cursor = sb;  // (this block may keep free slots above the ones taken)
                got += (uint32_t)__builtin_popcountll(fmask);
                if (got >= kb) break;
            }
            if (got < kb) {  // fewer free slots than visited rows: the host escalates and replays
                ovf = true;
                break;
            }
            taken += kb;
            minf = fin < minf ? fin : minf;
        }
        if (lane == 0) {
            mcs_vnode_result res;
            res.ok = (rc == 0u && rm == 0u) ? 1 : 0;
            res.visited = k;
            res.left_cores = rc;
            res.left_memory = rm;
            g.res[orig] = res;
            g.cnt[orig] = k;
        }
    }
    if (lane == 0) {
        if (ovf) atomicOr(&g.status->flags, (uint32_t)MCS_FLAG_OVERFLOW);
        if (taken != 0u) {  // (this wave alone writes its responder's state in this launch)
            cl->nrun += taken;
            cl->minf = minf < cl->minf ? minf : cl->minf;
            cl->l1_dirty = 1u;  // the commit may wrap a counter
        }
    }
}

// The Foreign records of the call, in array order and in row order within a request.  Every block scans
// the visit counts itself (at most 4096 of them) and writes the records of the requests i = block, block +
// grid, ...; block 0 moves the log's counter in the control block.
constexpr uint32_t kGrantMax = 4096;
__global__ __launch_bounds__(256) void dt_grant_log_kernel(DtArgs a, DtGrantArgs g) {
    __shared__ uint32_t excl[kGrantMax + 1];
    __shared__ uint32_t part[256];
    const uint32_t tid = threadIdx.x, n = g.n;
    if (g.status->flags & MCS_FLAG_OVERFLOW) return;  // (uniform: the walk ended before this launch)
    constexpr uint32_t kPer = kGrantMax / 256;
    uint32_t loc[kPer], sum = 0;
#pragma unroll
    for (uint32_t u = 0; u < kPer; ++u) {
        const uint32_t i = tid * kPer + u;
        loc[u] = i < n ? g.cnt[i] : 0u;
        sum += loc[u];
    }
    part[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        uint32_t run = 0;
        for (uint32_t t = 0; t < 256u; ++t) {
            const uint32_t x = part[t];
            part[t] = run;
            run += x;
        }
        excl[kGrantMax] = run;
    }
    __syncthreads();
    uint32_t run = part[tid];
#pragma unroll
    for (uint32_t u = 0; u < kPer; ++u) {
        excl[tid * kPer + u] = run;
        run += loc[u];
    }
    __syncthreads();
    const unsigned long long base = g.n_foreign;  // (the host's copy of the counter: no block reads what block 0 writes)
    const uint32_t total = excl[kGrantMax];
    bool lost = false;
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
        const uint32_t gi = g.inv[i];  // the request's place in the grouped arrays
        const mcs_vnode_request q = g.req[gi];
        const unsigned long long* stash = g.stash + 2ull * g.soff[gi];
        const uint32_t k = g.cnt[i];
        for (uint32_t j = tid; j < k; j += 256u) {
            const unsigned long long pos = base + excl[i] + j;
            if (pos < a.foreign_cap) {
                mcs_foreign_rec fr;
                fr.requester = q.requester;
                fr.responder = q.responder;
                fr.node = j;
                fr.start_s = g.T;
                fr.finish_s = g.T + q.time_s;
                fr.pad = 0u;
                fr.c = stash[2u * j];
                fr.m = stash[2u * j + 1u];
                a.foreign_log[pos] = fr;
            } else {
                lost = true;
            }
        }
    }
    if (lost) atomicOr(&g.status->flags, (uint32_t)MCS_FLAG_LOG_OVERFLOW);
    if (blockIdx.x == 0 && tid == 0) {
        g.status->n_foreign = base + total;
        g.status->added = total;
        a.ctl->n_foreign = base + total;
        if (base + total > a.foreign_cap) {  // beyond foreign_cap the records are counted, as the batch run does
            atomicOr(&g.status->flags, (uint32_t)MCS_FLAG_LOG_OVERFLOW);
            a.ctl->flags |= MCS_FLAG_LOG_OVERFLOW;
        }
    }
}

// AddVirtualNode (cluster.go:65-85) for the entries of one cluster, in array order: row nv + i takes
// entry i with capacity = free = the node's
__global__ __launch_bounds__(64) void dt_grant_recv_kernel(DtArgs a, DtGrantArgs g) {
    const uint32_t grp = blockIdx.x, lane = threadIdx.x;
    if (grp >= g.n_groups) return;
    const DtGrantGroup gr = g.groups[grp];
    const uint32_t c = gr.cluster, m = gr.end - gr.begin;
    DtCluster* cl = &a.cl[c];
    uint32_t nv0 = cl->nv;
    nv0 = nv0 < a.V ? nv0 : a.V;
    const uint32_t room = a.V - nv0, put = m < room ? m : room;
    for (uint32_t i = lane; i < put; i += kWave) {
        const mcs_vnode_grant nd = g.node[gr.begin + i];
        const size_t at = (size_t)c * a.V + nv0 + i;
        __hip_atomic_store(&a.vn[at], (unsigned long long)nd.cores | ((unsigned long long)nd.memory << 32),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        a.vcap[at] = make_uint2(nd.cores, nd.memory);
    }
    if (lane == 0) {
        if (put < m) atomicOr(&g.status->flags, (uint32_t)MCS_FLAG_VNODE_OVERFLOW);
        if (put != 0u) {
            cl->nv = nv0 + put;
            cl->l1_dirty = 1u;
            a.nv_all[a.base + c] = nv0 + put;
        }
    }
}

}  // namespace

hipError_t launch_dtrade_grant_provide(const DtArgs& a, const DtGrantArgs& g, hipStream_t s) {
    if (g.n == 0 || g.n > kGrantMax) return g.n == 0 ? hipSuccess : hipErrorInvalidValue;
    hipLaunchKernelGGL(dt_grant_walk_kernel, dim3(g.n_groups), dim3(kWave), 0, s, a, g);
    hipError_t st = hipGetLastError();
    if (st != hipSuccess) return st;
    const uint32_t nb = g.n < 64u ? g.n : 64u;
    hipLaunchKernelGGL(dt_grant_log_kernel, dim3(nb), dim3(256), 0, s, a, g);
    return hipGetLastError();
}

hipError_t launch_dtrade_grant_receive(const DtArgs& a, const DtGrantArgs& g, hipStream_t s) {
    if (g.n == 0) return hipSuccess;
    hipLaunchKernelGGL(dt_grant_recv_kernel, dim3(g.n_groups), dim3(kWave), 0, s, a, g);
    return hipGetLastError();
}

}  // namespace mcs
