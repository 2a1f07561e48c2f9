// TEST HARNESS -- host check of the walk's sigma' shortcut at a flat alpha jet
// (wost_device.h flat_alpha_min, flat_lane, flat_sigma_trivial). Built and run by
// tests/test_flat_sigma.py.
//
// For a lane the predicate calls trivial, the device's literal sequence --
// sigma_prime_from on the jet {a, 0, 0, 0} with sigma = 0, then the collision weight
// sc = 1 - sigma' * inv_sb in the reference form max(0, .) and the signed form of
// compat="fixed" -- must give 1.0f bit for bit. The device's divisions are a * rcp(b) with
// v_rcp_f32 within 1 ulp of 1/b, so the sequence is restated here with the reciprocal as
// an argument and run at RN(1/a) and at its two neighbours; the product sigma' * inv_sb is
// taken both rounded on its own and fused into the subtraction (the header allows the
// contraction within an expression).
//
// Swept per 1/sigma_bar: every float a from the bound to the end of the second binade above
// the bound's, and 4096 evenly spaced mantissas plus the first and last float of every
// higher binade up to FLT_MAX, and +inf. The rest follows from monotonicity: RN(1/a) and
// its neighbours do not increase with a, nor does any rounded product with a non-negative
// constant, so sigma' * |inv_sb| at any a is at most its value at a swept a below it.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

#include "../../dcrmontecarlo_amd/csrc/wost_device.h"

static uint32_t fb(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static float bf(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }

// wost::sigma_prime_from with the device's f_div(a, b) = a * rcp(b): y stands for rcp(ac),
// y2 for rcp(ac + 1e-8f). Every operation is rounded on its own (this file is built with
// -ffp-contract=off); the sums that the device may fuse add exact zeros here.
static float literal_sigma_prime(const wost::Jet& alpha, float sigma, float y, float y2) {
    const float ac = alpha.v < 1e-8f ? 1e-8f : alpha.v;
    const float ratio = sigma * y;
    const bool clamped = !(alpha.v >= 1e-8f);
    const float gx = clamped ? 0.f : alpha.gx, gy = clamped ? 0.f : alpha.gy;
    const float lap = 1e-8f + (clamped ? 0.f : alpha.lap);
    const float acp = ac + 1e-8f;
    const float rden = acp != ac ? y2 : y;
    const float lx = gx * rden, ly = gy * rden;
    const float gn = lx * lx + ly * ly;
    return ratio + 0.5f * (lap * y - gn / 2.0f);
}

struct Counts { long bad = 0, alphas = 0, evals = 0; };

// one trivial alpha: three reciprocals, two product forms, two weight forms
static void one(float a, float inv_sb, Counts& c) {
    ++c.alphas;
    const wost::Jet j{a, 0.0f, 0.0f, 0.0f};
    const float r = 1.0f / a, r2 = 1.0f / (a + 1e-8f);
    const float ys[3] = {bf(fb(r) - 1u), r, bf(fb(r) + 1u)};       // (r = +0 at a = inf: -min, 0, +min)
    const float y2s[3] = {bf(fb(r2) - 1u), r2, bf(fb(r2) + 1u)};
    for (int k = 0; k < 3; ++k) {
        const float y = k == 0 && fb(r) == 0u ? -bf(1u) : ys[k];
        const float y2 = k == 0 && fb(r2) == 0u ? -bf(1u) : y2s[k];
        const float sp = literal_sigma_prime(j, 0.0f, y, y2);
        const float signed_rounded = 1.0f - sp * inv_sb;            // compat="fixed": kept signed
        const float signed_fused = fmaf(-sp, inv_sb, 1.0f);
        const float max_rounded = (0.0f > signed_rounded) ? 0.0f : signed_rounded;   // Python max(., 0.0)
        const float max_fused = (0.0f > signed_fused) ? 0.0f : signed_fused;
        c.evals += 4;
        c.bad += (fb(signed_rounded) != 0x3F800000u) + (fb(signed_fused) != 0x3F800000u) +
                 (fb(max_rounded) != 0x3F800000u) + (fb(max_fused) != 0x3F800000u);
    }
    // the header's own function (IEEE divisions on the host)
    const float sph = wost::sigma_prime_from(j, 0.0f, false);
    c.evals += 1;
    c.bad += fb(1.0f - sph * inv_sb) != 0x3F800000u;
}

static void sweep(float inv_sb, uint32_t lo, uint32_t hi, Counts* out) {
    Counts c;
    for (uint32_t u = lo; u < hi; ++u) one(bf(u), inv_sb, c);
    *out = c;
}

// counts: [0] mismatches, [1] alphas swept, [2] evaluations, [3] predicate errors,
// [4] predicate checks
extern "C" int flat_sigma_check(long* counts) {
    const float inf = __builtin_inff(), nan = __builtin_nanf("");
    const float inv_sbs[] = {1e-3f, 0.1f, 1.0f, 10.0f, 1e3f, -0.1f};
    Counts total;
    long pred_bad = 0, pred_n = 0;
    auto expect = [&](bool got, bool want) { ++pred_n; pred_bad += got != want; };
    for (float inv_sb : inv_sbs) {
        const float amin = wost::flat_alpha_min(inv_sb);
        expect(amin >= 1e-8f && amin < inf, true);
        // the dense part: from the bound to the end of the second binade above its own
        const uint32_t lo = fb(amin), dense_end = ((lo >> 23) + 3u) << 23;
        unsigned nt = std::thread::hardware_concurrency();
        nt = nt < 1 ? 1 : nt > 16 ? 16 : nt;
        std::vector<Counts> part(nt);
        std::vector<std::thread> th;
        const uint64_t n = dense_end - lo;
        for (unsigned t = 0; t < nt; ++t)
            th.emplace_back(sweep, inv_sb, lo + (uint32_t)(n * t / nt), lo + (uint32_t)(n * (t + 1) / nt), &part[t]);
        for (auto& t : th) t.join();
        for (const Counts& p : part) { total.bad += p.bad; total.alphas += p.alphas; total.evals += p.evals; }
        // every higher binade: its first and last float and 4096 mantissas between
        for (uint32_t e = dense_end >> 23; e <= 254u; ++e) {
            for (uint32_t m = 0; m < (1u << 23); m += 1u << 11) one(bf((e << 23) | m), inv_sb, total);
            one(bf((e << 23) | 0x7FFFFFu), inv_sb, total);
        }
        one(inf, inv_sb, total);

        // the predicate: true from the bound on, false below it and for what is not a flat lane
        expect(wost::flat_sigma_trivial(true, amin, amin), true);
        expect(wost::flat_sigma_trivial(true, 0x1.fffffep+127f, amin), true);
        expect(wost::flat_sigma_trivial(true, inf, amin), true);
        expect(wost::flat_sigma_trivial(true, bf(lo - 1u), amin), false);   // just below the bound
        expect(wost::flat_sigma_trivial(true, nan, amin), false);
        expect(wost::flat_sigma_trivial(true, -amin, amin), false);
        expect(wost::flat_sigma_trivial(true, 9e-9f, amin), false);         // below the clamp
        expect(wost::flat_sigma_trivial(true, 0.0f, amin), false);
        expect(wost::flat_sigma_trivial(false, 1e3f, amin), false);         // the jet's full path ran
        // a radial factor's centre: the saturated jet's z is NaN, and the lane is not flat
        expect(wost::flat_lane(nan), false);
        expect(wost::flat_sigma_trivial(wost::flat_lane(nan), 1e3f, amin), false);
        expect(wost::flat_lane(0.0f), true);
        expect(wost::flat_sigma_trivial(wost::flat_lane(0.0f), 1e3f, amin), true);
    }
    // a bound below the clamp is the clamp; an unusable 1/sigma_bar makes no lane trivial
    expect(wost::flat_alpha_min(1e-9f) == 1e-8f, true);
    expect(wost::flat_sigma_trivial(true, 9.9e-9f, wost::flat_alpha_min(1e-9f)), false);
    expect(wost::flat_alpha_min(0.0f) == 1e-8f, true);
    for (float bad : {inf, -inf, nan, 0x1p65f, -0x1p100f}) {
        const float amin = wost::flat_alpha_min(bad);
        expect(amin != amin, true);
        for (float a : {1e-8f, 1.0f, 0x1.fffffep+127f, inf}) expect(wost::flat_sigma_trivial(true, a, amin), false);
    }
    one(1e-8f, 1e-9f, total);   // the clamp itself as the bound

    counts[0] = total.bad;
    counts[1] = total.alphas;
    counts[2] = total.evals;
    counts[3] = pred_bad;
    counts[4] = pred_n;
    return 0;
}
