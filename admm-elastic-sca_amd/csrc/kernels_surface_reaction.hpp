// kernels_surface_reaction.hpp -- two-way contact on the device (surface_reaction.hpp): per frame, behind the reaction and attribution
// chain of kernels_reaction.hpp (reaction_elem_kernel, reaction_gather_kernel, contact_count / row_scan / contact_scatter_kernel,
// contact_owner_scatter_kernel, all launched unchanged), the contacts that landed on a body or sheet surface with a share hand
// -f to the corners of the triangle they landed on.  Extension, no reference counterpart; launched by admm_hip_step only while some
// surface has a share above zero (abi_surface_reaction.inc).  No float atomics and no integer atomics anywhere: every contribution is
// stored once, then summed per destination through an inverted index with a fixed order, so two runs give the same bits and the
// device gives admm_hip_surface_reaction_query's.  The contact count K never leaves the device: every grid is sized by the host-known
// capacity (the nodes that carry a collision element), a block beyond the device's count returns after one load.
//
// surface_share_kernel   one lane: a surface's share, from a kernel argument, into the table the hit kernel reads (no host buffer has to
//                        outlive the call that set it)
// surface_clear_kernel   one lane per sorted share of the PREVIOUS reacting frame: the first lane of a run writes 0.0 to its node's dv,
//                        so dv is exactly 0.0 where nothing lands without a pass over all nodes
// surface_hit_kernel     one lane per contact k < K, SR_BLOCK = 64: classifies the contact (surface_reaction.hpp classify); a reacting
//                        one takes its point to the entry's coordinates, runs the unbounded BVH query (mesh_query.hpp closest, the
//                        traversal stack in the lane's LDS column) and tri_weights; writes the 64-byte record and three shares
//                        (key = destination node in the caller's order, value = g p[3]); a contact that does not react writes the
//                        sentinel key n_nodes, which sorts last.  Lane 0 of block 0 leaves 3 K on the device for the kernels behind it.
//                        The frame and translation of the entry are taken off as the collision rule does; today the library refuses
//                        both on an entry that names a surface of simulated nodes (abi_setup.inc check_body_entries), so for a
//                        reacting contact they are the identity and zero, and those two lines change no bit.  K is clamped to the
//                        buffers' capacity as a bound on the writes; abi_surface_reaction.inc says why the clamp never acts.
// surface_info_kernel    one wave, launched by the report and not by the step: the counts by status over the K records
// The inverted index: a stable LSD radix sort of the 3 K keys, 8 bits per pass, the number of passes from the key range
// (surface_reaction.hpp sort_passes), three launches per pass, no spinning across workgroups:
//   sort_count_kernel    one wave per 64 keys: the lanes with the same digit find each other with eight ballots (one per bit of the
//                        digit), the lowest of them writes their number to an LDS histogram of 256 digits; counts [256][blocks]
//   sort_scan_kernel     one wave per digit: kernels_reaction.hpp's wave_scan_row over that digit's block counts -> block offsets, total
//   sort_place_kernel    the count kernel's ballots again; a key's place = (the totals of the lower digits: wave_scan_inclusive over the
//                        256 totals, four per lane, into LDS) + its block's offset + its rank among the lanes with the same digit; moves the key and the index
//                        it carries.  Equal keys keep their order: ascending block, then ascending lane.
// After the last pass a node's shares are adjacent, in ascending (contact k, corner c): the order surface_reaction.hpp demands.
// surface_apply_kernel   one lane per sorted share: the lane at the start of a run (the key before differs) walks its run in sorted order,
//                        a = 0.0; a = a + q, then dv = a / m, v = v - dv on the node's device position.  Runs are short in practice (the
//                        contacts around one surface vertex); a long run is walked by one lane.
//
// Cost: not measured, no timing claimed.  Expected to be bound by memory and launch count: per pass a key is read twice and moved once
// with its index (16 B), a block writes and reads 2 KiB of counts; the hit kernel adds one divergent BVH walk per reacting contact
// (about the depth of the tree in 64-byte nodes plus a few leaves of 96-byte triangles); per frame O(K passes + the vertices that
// received a share), never K x vertices.
#pragma once
#include "kernels_reaction.hpp"
#include "surface_reaction.hpp"
#include "mesh_query.hpp"
#include "frame.hpp"

namespace admm_dev {

constexpr int SR_BLOCK = 64, SR_DIGITS = 256;
static_assert(SR_BLOCK == 64 && SR_DIGITS == 4 * SR_BLOCK, "one wave per block, four digits per lane");

// per registered mesh, parallel to admm_hip_ctx::d_meshes: the caller's node id of every vertex (null: not a surface of simulated
// nodes) and the surface's share
struct SrMesh { const int *vnode; double share; };

struct SrStack { int *col; __device__ int &operator[](int i) { return col[i * SR_BLOCK]; } };

__global__ void surface_share_kernel(SrMesh *__restrict__ sm, const int mesh, const double share) {
    if (blockIdx.x == 0 && threadIdx.x == 0) sm[mesh].share = share;
}

__global__ __launch_bounds__(SR_BLOCK) void surface_clear_kernel(const long long *__restrict__ n_shares, const int *__restrict__ skey, const int sentinel, double *__restrict__ dv) {
    const long long i = (long long)blockIdx.x * SR_BLOCK + threadIdx.x;
    if (i >= *n_shares) return;
    const int key = skey[i];
    if (key >= sentinel || (i > 0 && skey[i - 1] == key)) return;
    dv[3 * (size_t)key] = 0.0; dv[3 * (size_t)key + 1] = 0.0; dv[3 * (size_t)key + 2] = 0.0;
}

// crec, orec: the contact and owner records of the same compaction; tag: the owner group of every node in device order (null: no
// owners), iperm: caller's node -> device position; capacity: the records and shares the buffers hold
__global__ __launch_bounds__(SR_BLOCK) void surface_hit_kernel(const long long *__restrict__ count, const ContactRecord *__restrict__ crec, const OwnerRecord *__restrict__ orec,
                                                               const ShapeTable *__restrict__ shapes, const admm_mesh::MeshDev *__restrict__ meshes,
                                                               const admm_mesh::MeshMotion *__restrict__ mm, const SrMesh *__restrict__ sm, const int *__restrict__ tag,
                                                               const int *__restrict__ iperm, const double dt, const int sentinel, const long long capacity,
                                                               admm_surface_reaction::Record *__restrict__ rec, int *__restrict__ key, int *__restrict__ idx,
                                                               double *__restrict__ val, long long *__restrict__ n_shares) {
    using namespace admm_surface_reaction;
    __shared__ int stack[admm_mesh::MAX_DEPTH][SR_BLOCK];
    const long long K = *count < capacity ? *count : capacity;
    const long long k = (long long)blockIdx.x * SR_BLOCK + threadIdx.x;
    if (k == 0) *n_shares = 3 * K;
    if (k >= K) return;
    const ContactRecord c = crec[k];
    const int entry = orec[k].entry;
    Record r;
    r.node = c.node; r.mesh = -1; r.tri = -1; r.corner[0] = r.corner[1] = r.corner[2] = -1; r.pad_ = 0;
    r.weight[0] = r.weight[1] = r.weight[2] = 0.0; r.share = 0.0;
    int mi = -1;
    bool surface = false, own = false;
    double share = 0.0;
    if (entry >= 0 && entry < shapes->n && shapes->type[entry] == ADMM_SHAPE_MESH) {
        mi = (int)shapes->par[entry][3];
        r.mesh = mi;
        surface = sm[mi].vnode != nullptr;
        share = sm[mi].share;
        const int o = meshes[mi].owner;
        own = tag && o >= 0 && tag[iperm[c.node]] == o;
    }
    r.status = classify(entry, surface, share, own);
    int dest[3] = {sentinel, sentinel, sentinel};
    double q[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    if (r.status == REACTING) {
        const admm_mesh::MeshDev m = meshes[mi];
        const double *f = shapes->frame[entry];
        double l[3] = {c.point[0], c.point[1], c.point[2]};
        if (shapes->framed[entry] != 0) admm_frame::to_local(f, c.point, l);
        const double qq[3] = {l[0] - shapes->par[entry][0], l[1] - shapes->par[entry][1], l[2] - shapes->par[entry][2]};
        SrStack stk{&stack[0][threadIdx.x]};
        admm_mesh::Hit h;
        admm_mesh::closest(m.nodes, m.tris, qq, stk, h);
        if (h.slot >= 0) {
            const admm_mesh::Tri &tr = m.tris[h.slot];
            const int *cv = mm[mi].cid + 3 * (size_t)tr.orig;
            admm_mesh::tri_weights(qq, tr.v, h.reg, r.weight);
            r.tri = tr.orig; r.share = share;
            double p[3];
            impulse(dt, c.f, p);
            for (int cc = 0; cc < 3; ++cc) {
                dest[cc] = sm[mi].vnode[cv[cc]];
                r.corner[cc] = dest[cc];
                contribution(share, r.weight[cc], p, q[cc]);
            }
        } else r.status = OTHER;      // (a mesh without triangles cannot be registered: not reached)
    }
    rec[k] = r;
    for (int cc = 0; cc < 3; ++cc) {
        const long long s = 3 * k + cc;
        key[s] = dest[cc]; idx[s] = (int)s;
        val[3 * s] = q[cc][0]; val[3 * s + 1] = q[cc][1]; val[3 * s + 2] = q[cc][2];
    }
}

// the report's counts {contacts, reacting, unowned, other, self} over the K records of the last reacting frame; one wave, a ballot per
// status and chunk of 64 records (launched by admm_hip_get_surface_reaction, not by the step)
__global__ __launch_bounds__(SR_BLOCK) void surface_info_kernel(const long long *__restrict__ n_shares, const admm_surface_reaction::Record *__restrict__ rec,
                                                                long long *__restrict__ info) {
    const long long K = *n_shares / 3;
    const int lane = threadIdx.x;
    long long c[4] = {0, 0, 0, 0};
    for (long long base = 0; base < K; base += SR_BLOCK) {      // (uniform: every lane runs every chunk)
        const long long k = base + lane;
        const int st = k < K ? rec[k].status : -1;
#pragma unroll
        for (int q = 0; q < 4; ++q) c[q] += __popcll(__ballot(st == q));
    }
    if (lane == 0) {
        info[0] = K; info[1] = c[admm_surface_reaction::REACTING]; info[2] = c[admm_surface_reaction::UNOWNED];
        info[3] = c[admm_surface_reaction::OTHER]; info[4] = c[admm_surface_reaction::SELF];
    }
}

// the lanes of the wave that hold the same digit as this one (valid lanes only); 8 ballots, one per bit
__device__ __forceinline__ unsigned long long sort_peers(const bool valid, const int digit) {
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const bool bit = ((digit >> b) & 1) != 0;
        const unsigned long long bal = __ballot(valid && bit);
        peers &= bit ? bal : ~bal;
    }
    return peers;
}

// blk_count [SR_DIGITS][nb_stride]: the keys of block b with digit d = (key >> shift) & 255
__global__ __launch_bounds__(SR_BLOCK) void sort_count_kernel(const long long *__restrict__ n, const int *__restrict__ key_in, const int shift, const int nb_stride,
                                                              int *__restrict__ blk_count) {
    __shared__ int hist[SR_DIGITS];
    const long long N = *n, base = (long long)blockIdx.x * SR_BLOCK;
    if (base >= N) return;      // (uniform across the block)
    const int lane = threadIdx.x;
    const bool valid = base + lane < N;
    const int digit = valid ? (key_in[base + lane] >> shift) & (SR_DIGITS - 1) : 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) hist[4 * lane + q] = 0;
    __syncthreads();
    const unsigned long long peers = sort_peers(valid, digit);
    if (valid && (peers & ((1ull << lane) - 1ull)) == 0ull) hist[digit] = __popcll(peers);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) blk_count[(size_t)(4 * lane + q) * nb_stride + blockIdx.x] = hist[4 * lane + q];
}

// digit blockIdx.x: wave_scan_row over its counts of the ceil(N / 64) blocks in use -> blk_off, total[digit]; one wave
__global__ __launch_bounds__(RX_SCAN) void sort_scan_kernel(const long long *__restrict__ n, const int nb_stride, const int *__restrict__ blk_count, int *__restrict__ blk_off,
                                                            int *__restrict__ total) {
    const int t = wave_scan_row((int)((*n + SR_BLOCK - 1) / SR_BLOCK), blk_count + (size_t)blockIdx.x * nb_stride, blk_off + (size_t)blockIdx.x * nb_stride);
    if (threadIdx.x == 0) total[blockIdx.x] = t;
}

__global__ __launch_bounds__(SR_BLOCK) void sort_place_kernel(const long long *__restrict__ n, const int *__restrict__ key_in, const int *__restrict__ idx_in, const int shift,
                                                              const int nb_stride, const int *__restrict__ blk_off, const int *__restrict__ total,
                                                              int *__restrict__ key_out, int *__restrict__ idx_out) {
    __shared__ int digit_base[SR_DIGITS];
    const long long N = *n, base = (long long)blockIdx.x * SR_BLOCK;
    if (base >= N) return;      // (uniform across the block)
    const int lane = threadIdx.x;
    {   // exclusive scan of the 256 totals: four per lane, then wave_scan_inclusive of the lanes' sums
        int t[4], s = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) { t[q] = total[4 * lane + q]; s += t[q]; }
        int run = wave_scan_inclusive(s, lane) - s;
#pragma unroll
        for (int q = 0; q < 4; ++q) { digit_base[4 * lane + q] = run; run += t[q]; }
    }
    __syncthreads();
    const bool valid = base + lane < N;
    const int k = valid ? key_in[base + lane] : 0;
    const int digit = (k >> shift) & (SR_DIGITS - 1);
    const unsigned long long peers = sort_peers(valid, digit);
    if (!valid) return;
    const long long pos = (long long)digit_base[digit] + blk_off[(size_t)digit * nb_stride + blockIdx.x] + __popcll(peers & ((1ull << lane) - 1ull));
    if (pos < N) { key_out[pos] = k; idx_out[pos] = idx_in[base + lane]; }      // (pos < N always: the counts add up to N)
}

// idx[i] = i for i < N (the debug entry's start; the hit kernel writes its own)
__global__ __launch_bounds__(SR_BLOCK) void sort_iota_kernel(const long long *__restrict__ n, int *__restrict__ idx) {
    const long long i = (long long)blockIdx.x * SR_BLOCK + threadIdx.x;
    if (i < *n) idx[i] = (int)i;
}

// skey, sidx: the sorted keys and the share each came from; val [3 K][3]; m3, v in device order; dv [n_nodes][3] in the caller's order
__global__ __launch_bounds__(SR_BLOCK) void surface_apply_kernel(const long long *__restrict__ n_shares, const int *__restrict__ skey, const int *__restrict__ sidx,
                                                                 const double *__restrict__ val, const int sentinel, const int *__restrict__ iperm,
                                                                 const double *__restrict__ m3, double *__restrict__ v, double *__restrict__ dv) {
    const long long N = *n_shares, i = (long long)blockIdx.x * SR_BLOCK + threadIdx.x;
    if (i >= N) return;
    const int key = skey[i];
    if (key >= sentinel || (i > 0 && skey[i - 1] == key)) return;
    double a[3] = {0.0, 0.0, 0.0};
    for (long long j = i; j < N && skey[j] == key; ++j) admm_surface_reaction::accumulate(val + 3 * (size_t)sidx[j], a);
    const size_t t = (size_t)iperm[key];
    const double m[3] = {m3[3 * t], m3[3 * t + 1], m3[3 * t + 2]};
    double vv[3] = {v[3 * t], v[3 * t + 1], v[3 * t + 2]}, d[3];
    admm_surface_reaction::apply(a, m, d, vv);
    for (int j = 0; j < 3; ++j) { v[3 * t + j] = vv[j]; dv[3 * (size_t)key + j] = d[j]; }
}

} // namespace admm_dev
