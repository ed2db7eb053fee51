// The host side of rigid attachments under AddressSanitizer + UBSan in a stand-alone program (tools/asan_attach.sh): attach_host.cpp's
// admm_hip_attachment_query, compiled into this program with the sanitizers, at the sizes where its block and lane loops end; and the
// registration calls and their refusals on a host-only context of the library as built (its allocations go through the sanitizer's
// allocator, so an overrun of a batch's offsets or targets on the heap is caught when the block is freed).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "admm_hip.h"

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "asan_attach: line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

int main() {
    // ---- the query: targets and sums, every size at which a loop of the two-stage sum ends
    const int sizes[] = {0, 1, 63, 64, 65, 130, 64 * 256, 64 * 257 + 3};
    const double c[3] = {0.5, -1.0, 2.0}, R[9] = {0.0, -1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0}, pivot[3] = {0.1, 0.2, 0.3};
    for (int n : sizes) {
        std::vector<double> local(3 * (size_t)n), targets(3 * (size_t)n), f(3 * (size_t)n), point(3 * (size_t)n);
        std::vector<int32_t> active((size_t)n);
        for (int i = 0; i < 3 * n; ++i) { local[i] = 0.001 * i; f[i] = std::sin(0.1 * i); point[i] = std::cos(0.07 * i); }
        for (int i = 0; i < n; ++i) active[i] = i % 5 != 0;
        double row[6]; int64_t na = -1;
        CHECK(admm_hip_attachment_query(n, c, R, local.data(), targets.data(), f.data(), point.data(), active.data(), pivot, row, &na) == ADMM_OK);
        int want = 0;
        for (int i = 0; i < n; ++i) want += active[i] != 0;
        CHECK(na == want);
        if (n) CHECK(targets[0] == c[0] + (R[0] * local[0] + (R[1] * local[1] + R[2] * local[2])));
        double sum = 0.0;
        for (int i = 0; i < n; ++i) if (active[i]) sum += f[3 * (size_t)i];
        CHECK(std::fabs(row[0] - sum) <= 1e-9 * (1.0 + n));
        CHECK(admm_hip_attachment_query(n, c, R, local.data(), nullptr, f.data(), point.data(), nullptr, nullptr, row, nullptr) == ADMM_OK);      // all active, about the origin
    }
    CHECK(admm_hip_attachment_query(-1, c, R, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == ADMM_ERR_ARG);
    double t3[3], r6[6];
    CHECK(admm_hip_attachment_query(1, c, R, nullptr, t3, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == ADMM_ERR_ARG);
    CHECK(admm_hip_attachment_query(1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, r6, nullptr) == ADMM_ERR_ARG);

    // ---- registration and its refusals on a host-only context: four nodes, one tet, a static and a moving anchor batch, a sphere as a body
    admm_hip_ctx *ctx = nullptr;
    CHECK(admm_hip_create(&ctx, -1) == ADMM_OK);
    const double x[12] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1}, m[12] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1};
    CHECK(admm_hip_add_nodes(ctx, 4, x, m, nullptr) == ADMM_OK);
    const int32_t tet[4] = {0, 1, 2, 3}; const double tpar[1] = {1e4};
    int bt = -1, bs = -1, bm = -1;
    CHECK(admm_hip_add_batch(ctx, ADMM_KIND_TET_LINEAR, 1, tet, tpar, nullptr, &bt) == ADMM_OK);
    const int32_t a0[1] = {0}, a1[2] = {2, 3}; const double ap[4] = {1000.0, 1.0, 1000.0, 1.0}, tg[6] = {0, 1, 0, 0, 0, 1};
    CHECK(admm_hip_add_batch(ctx, ADMM_KIND_ANCHOR, 1, a0, ap, nullptr, &bs) == ADMM_OK);
    CHECK(admm_hip_add_batch(ctx, ADMM_KIND_ANCHOR, 2, a1, ap, tg, &bm) == ADMM_OK);
    const int32_t ty[1] = {ADMM_SHAPE_SPHERE}; const double par[4] = {3.0, 0.0, 0.0, 0.5};
    CHECK(admm_hip_set_collision_shapes(ctx, 1, ty, par) == ADMM_OK);
    CHECK(admm_hip_enable_contact_attribution(ctx, 1) == ADMM_OK);
    CHECK(admm_hip_attach_anchors(ctx, bt, 0, nullptr) == ADMM_ERR_ARG);            // not an anchor batch
    CHECK(admm_hip_attach_anchors(ctx, 7, 0, nullptr) == ADMM_ERR_ARG);
    CHECK(admm_hip_attach_anchors(ctx, bm, 0, nullptr) == ADMM_ERR_ARG);            // no body yet
    const double J[6] = {0.1, 0, 0, 0.1, 0, 0.1}, com[3] = {3.0, 0.0, 0.0};
    int body = -1;
    CHECK(admm_hip_add_rigid_body(ctx, 0, 2.0, J, com, nullptr, &body) == ADMM_OK && body == 0);
    double bad[6] = {0, 0, 0, 0, NAN, 0};
    CHECK(admm_hip_attach_anchors(ctx, bm, body, bad) == ADMM_ERR_ARG);             // a non-finite offset
    CHECK(admm_hip_attach_anchors(ctx, bm, body, nullptr) == ADMM_OK);              // derived offsets
    CHECK(admm_hip_attach_anchors(ctx, bm, body, nullptr) == ADMM_ERR_ARG);         // attached already
    CHECK(admm_hip_attach_anchors(ctx, bs, body, nullptr) == ADMM_OK);              // a static batch: its node's position
    int got = -2; double loc[6], tgt[6];
    CHECK(admm_hip_get_attachment(ctx, bm, &got, loc, tgt) == ADMM_OK && got == body && loc[0] == tg[0] - com[0] && tgt[1] == tg[1]);
    CHECK(admm_hip_update_anchors(ctx, bm, tg, nullptr) == ADMM_ERR_STATE);
    const int32_t flags[2] = {1, 0};
    CHECK(admm_hip_update_anchors(ctx, bm, nullptr, flags) == ADMM_OK);
    CHECK(admm_hip_finalize(ctx) == ADMM_OK);
    double Fa[3], Ta[3]; int64_t na = -1;
    CHECK(admm_hip_get_attachment_load(ctx, 1, Fa, Ta, &na) == ADMM_OK && na == 0 && Fa[0] == 0.0);
    CHECK(admm_hip_get_attachment_load(ctx, 2, Fa, Ta, &na) == ADMM_ERR_ARG);
    CHECK(admm_hip_detach_anchors(ctx, bm) == ADMM_OK);
    CHECK(admm_hip_detach_anchors(ctx, bm) == ADMM_ERR_ARG);
    CHECK(admm_hip_update_anchors(ctx, bm, tg, nullptr) == ADMM_OK);
    CHECK(admm_hip_get_attachment(ctx, bm, &got, loc, nullptr) == ADMM_OK && got == -1 && loc[0] == 0.0);
    admm_hip_destroy(ctx);
    std::printf("asan_attach: ok\n");
    return 0;
}
