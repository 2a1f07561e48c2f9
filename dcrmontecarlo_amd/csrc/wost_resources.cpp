// wost_resources.cpp -- what a handle builds once and keeps on the device: the sampler /
// G_norm table (with the process-wide sampler-node cache and its prefetch thread), the
// Neumann segment tree, the field program and the point charges.
#include <algorithm>
#include <condition_variable>
#include <map>
#include <mutex>
#include <set>
#include <thread>

#include "wost_handle.h"
#include "wost_tables.h"

namespace wost {

int upload_program(wost_handle* h) {
    if (!h->prog_dirty) return WOST_OK;
    build_program(h->fields, h->sigma_bar, h->prog, &h->model_fields);
    HIP_TRY(h->d_prog.reserve(h->prog.bytes.size()));
    HIP_TRY(hipMemcpy(h->d_prog, h->prog.bytes.data(), h->prog.bytes.size(), hipMemcpyHostToDevice));
    h->prog_dirty = false;
    ++h->prog_version;
    return WOST_OK;
}

// The corrected screened sampler's nodes do not depend on sigma_bar (only on the
// shape s = R sqrt(sigma_bar)): built once per process (~0.5 s of Bessel series).
const std::vector<float>& fixed_screened_table() {
    static const std::vector<float> t = [] {
        std::vector<float> v((size_t)kFixTableFloats);
        screened_fixed_nodes(v.data(), kFixRows, kFixCols, kFixXMax);
        return v;
    }();
    return t;
}

namespace {

// The radial sampler's nodes depend only on the sampler and (screened) sigma_bar: each
// table is computed once per process (8-14 ms of host time, which every fresh handle's
// first solve paid; a survey's handles share one sigma_bar). kind: sampler_kind.
// (the cache and its lock are never destroyed: a prefetch thread may outlive the statics)
struct NodeCache {
    std::mutex mu;
    std::condition_variable cv;
    std::map<std::pair<int, uint64_t>, std::vector<float>> done;
    std::set<std::pair<int, uint64_t>> running;
};
NodeCache& node_cache() {
    static NodeCache* c = new NodeCache;
    return *c;
}

std::pair<int, uint64_t> node_key(int kind, double sigma_bar) {
    uint64_t bits = 0;
    if (kind == 2) std::memcpy(&bits, &sigma_bar, sizeof(bits));
    return std::make_pair(kind, bits);
}

void compute_nodes(int kind, double sigma_bar, std::vector<float>& v) {
    v.resize(WOST_SAMPLER_TABLE_N);
    if (kind == 2) screened_sampler_nodes(v.data(), WOST_SAMPLER_TABLE_N, sigma_bar);
    else if (kind == 1) greens_sampler_nodes_jacobian(v.data(), WOST_SAMPLER_TABLE_N);
    else greens_sampler_nodes(v.data(), WOST_SAMPLER_TABLE_N);
}

void store_nodes(const std::pair<int, uint64_t>& key, std::vector<float>&& v) {
    NodeCache& c = node_cache();
    std::lock_guard<std::mutex> lock(c.mu);
    if (c.done.size() >= 64) c.done.clear();
    c.done.emplace(key, std::move(v));
    c.running.erase(key);
    c.cv.notify_all();
}

void sampler_nodes_once(int kind, double sigma_bar, float* out) {
    NodeCache& c = node_cache();
    const auto key = node_key(kind, sigma_bar);
    {
        std::unique_lock<std::mutex> lock(c.mu);
        c.cv.wait(lock, [&] { return !c.running.count(key); });   // (a prefetch computing them)
        auto it = c.done.find(key);
        if (it != c.done.end()) {
            std::memcpy(out, it->second.data(), sizeof(float) * WOST_SAMPLER_TABLE_N);
            return;
        }
        c.running.insert(key);
    }
    std::vector<float> v;
    compute_nodes(kind, sigma_bar, v);
    std::memcpy(out, v.data(), sizeof(float) * WOST_SAMPLER_TABLE_N);
    store_nodes(key, std::move(v));
}

}  // namespace

// wost_create: the nodes a first solve of this handle needs, computed in the background
// while the handle's device setup runs (a fresh process's first HIP calls take ~0.1 s).
void sampler_nodes_prefetch(int kind, double sigma_bar) {
    NodeCache& c = node_cache();
    const auto key = node_key(kind, sigma_bar);
    {
        std::lock_guard<std::mutex> lock(c.mu);
        if (c.running.count(key) || c.done.count(key)) return;
        c.running.insert(key);
    }
    try {
        std::thread([kind, sigma_bar, key]() {
            std::vector<float> v;
            compute_nodes(kind, sigma_bar, v);
            store_nodes(key, std::move(v));
        }).detach();
    } catch (...) {
        std::vector<float> v;
        compute_nodes(kind, sigma_bar, v);
        store_nodes(key, std::move(v));
    }
}

int ensure_table(wost_handle* h) {
    if (h->table_ready) return WOST_OK;
    // sampler nodes (compat="fixed" delta tracking: staged, unused), then (delta tracking)
    // the G_norm cells (wost_device.h), then (compat="fixed" delta tracking) the corrected
    // screened sampler's nodes
    const bool fix_delta = h->delta && h->compat == WOST_COMPAT_FIXED;
    const size_t n = table_floats(h->delta, fix_delta);
    h->table.assign(n, 0.f);
    const int kind = sampler_kind(h);
    sampler_nodes_once(kind, kind == 2 ? h->sigma_bar : 0.0, h->table.data());
    if (h->delta)
        greens_norm_cells(h->table.data() + kSamplerFloatsPadded, kGnormCells, (double)kGnormCells / kGnormInvH);
    if (fix_delta) {
        const std::vector<float>& fx = fixed_screened_table();
        std::memcpy(h->table.data() + kFixTableOffset, fx.data(), sizeof(float) * fx.size());
    }
    HIP_TRY(h->d_table.reserve(std::max(n, table_floats(true))));
    HIP_TRY(hipMemcpy(h->d_table, h->table.data(), sizeof(float) * n, hipMemcpyHostToDevice));
    h->table_ready = true;
    return WOST_OK;
}

int ensure_tree(wost_handle* h) {
    if (h->tree_ready) return WOST_OK;
    const int nv = (int)(h->nverts.size() / 2);
    // a polyline too long for kTreeMaxDepth levels at the chosen leaf size takes 32 per leaf
    if (!build_segment_tree(h->nverts.data(), nv, h->tree_leaf, &h->tree) &&
        !build_segment_tree(h->nverts.data(), nv, 32, &h->tree))
        return fail(WOST_ERR_UNSUPPORTED, "cannot build the Neumann segment tree of %d segments (at most %d levels "
                    "of 32-segment leaves)", nv - 1, kTreeMaxDepth);
    HIP_TRY(h->d_tree.reserve(std::max<size_t>(h->tree.rec.size(), 16)));
    if (!h->tree.rec.empty())
        HIP_TRY(hipMemcpy(h->d_tree, h->tree.rec.data(), sizeof(float) * h->tree.rec.size(), hipMemcpyHostToDevice));
    h->tree_ready = true;
    return WOST_OK;
}

// The Dirichlet tree of a handle whose polyline admits it (use_dtree), built and uploaded on
// first use; the same fallback as ensure_tree when the builder refuses the leaf size.
int ensure_dtree(wost_handle* h) {
    if (h->dtree_ready) return WOST_OK;
    const int nv = (int)(h->dverts.size() / 2);
    if (!build_segment_tree(h->dverts.data(), nv, h->dtree_leaf, &h->dtree) &&
        !build_segment_tree(h->dverts.data(), nv, 32, &h->dtree))
        return fail(WOST_ERR_UNSUPPORTED, "cannot build the Dirichlet segment tree of %d segments (at most %d levels "
                    "of 32-segment leaves)", nv - 1, kTreeMaxDepth);
    HIP_TRY(h->d_dtree.reserve(std::max<size_t>(h->dtree.rec.size(), 16)));
    if (!h->dtree.rec.empty())
        HIP_TRY(hipMemcpy(h->d_dtree, h->dtree.rec.data(), sizeof(float) * h->dtree.rec.size(), hipMemcpyHostToDevice));
    h->dtree_ready = true;
    return WOST_OK;
}

// The device image of the handle's charges (WalkArgs::charges), alpha left at 1.
int upload_charges(wost_handle* h) {
    std::vector<float> w((size_t)kChargeWords, 0.0f);
    for (size_t p = 0; p < h->charges.size(); ++p) {
        const wost_point_charge& c = h->charges[p];
        w[CHG_XY + 2 * p] = c.x;
        w[CHG_XY + 2 * p + 1] = c.y;
        w[CHG_Q + p] = c.strength;
        w[CHG_ALPHA + p] = 1.0f;
        std::memcpy(&w[CHG_SOURCE + p], &c.source, sizeof(int32_t));
        std::memcpy(&w[CHG_SEG0 + p], &h->charge_seg[2 * p], sizeof(int32_t));
        std::memcpy(&w[CHG_SEG1 + p], &h->charge_seg[2 * p + 1], sizeof(int32_t));
    }
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(h->d_charges.reserve((size_t)kChargeWords));
    HIP_TRY(hipMemcpy(h->d_charges, w.data(), sizeof(float) * w.size(), hipMemcpyHostToDevice));
    return WOST_OK;
}

}  // namespace wost
