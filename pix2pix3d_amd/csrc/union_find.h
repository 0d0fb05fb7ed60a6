// Lock-free union-find on an int32 parent array in global memory (ECL-CC shape: Jaiganesh & Burtscher, HPDC 2018), shared by
// csrc/mesh_ops.hip (components of a mesh) and csrc/regions/label_regions.hip (components of a label map).
// Every write keeps parent[x] <= x and parent[x] inside x's own component:
//   * a hook is atomicCAS(&parent[hi], hi, lo) with lo < hi the two roots an edge joins: only a ROOT is ever hooked, and under a
//     smaller id, so the root of a finished tree is the smallest id of its component whatever the order of arrival;
//   * path halving while finding stores an ancestor of x into parent[x] for a NON-root x; two such stores may race, both are ancestors.
// A failed CAS means parent[hi] != hi: some other thread hooked hi, the component count went down, and this thread goes on from the
// value the CAS returned (an ancestor).  Nothing waits for a value another thread has yet to write: no locks, no spinning on a flag, so
// lanes of one wave that run in lockstep cannot starve each other.  Reads of parent[] go through relaxed agent-scope atomics (the
// XCDs' L2s are not coherent for plain accesses inside one kernel); a stale read returns an older ancestor, which the loop tolerates.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace p3d {

__device__ __forceinline__ int32_t uf_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void uf_store(int32_t* p, int32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The root of v's tree, halving the path on the way: every visited vertex is pointed at its grandparent.  Terminates because
// parent[x] <= x, with equality only at a root.
__device__ __forceinline__ int32_t uf_find(int32_t* parent, int32_t v)
{
    int32_t cur = uf_load(parent + v);
    if (cur == v) return v;
    int32_t prev = v, next;
    while (cur > (next = uf_load(parent + cur))) {
        uf_store(parent + prev, next);
        prev = cur;
        cur = next;
    }
    return cur;
}

__device__ __forceinline__ void uf_union(int32_t* parent, int32_t a, int32_t b)
{
    int32_t ra = uf_find(parent, a), rb = uf_find(parent, b);
    while (ra != rb) {
        const int32_t hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
        const int32_t seen = atomicCAS(parent + hi, hi, lo);
        if (seen == hi) return;                                      // hooked
        ra = seen; rb = lo;                                          // hi was hooked by somebody else: go on from its new parent (< hi)
    }
}

} // namespace p3d
