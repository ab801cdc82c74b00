/* A C ABI caller with a 3D batch WITHOUT normals (rxr_batch3d.clipped_normals == NULL), on a machine WITH a GPU -- the host mirror refuses
 * such batches as the reference panics on them, the C ABI takes them.  A small host-projected frame of two batches: the first carries
 * normals, the second does not, so its vertices index a part of the normals pool that rxr_upload_frame never writes -- and which a frame
 * uploaded just before has left full of sevens in the staging blob.  The set-up records rxr_upload_frame makes on the host must equal
 * the ones k_setup3d writes, all n x 96 and n x 80 bytes (rxr_debug_setup_records; no coordinate here is special, so the bytes are
 * compared as they are), with zero normals in the second batch's records.  One vertex of the first batch has w = 0, a vertex on the eye
 * plane: its 1 / w and uv / w are +inf in both sets of records.  And the frame rendered from them (a context created under
 * RXR_HOST_SETUP=1) must equal the frame of a context created under RXR_HOST_SETUP=0, which launches k_setup3d.
 * Run by tests/test_gpu_abi_no_normals.py (gcc -std=c11 -Wall -Werror). */
#define _POSIX_C_SOURCE 200112L
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../rusterix_amd/csrc/rxr_debug.h" /* rxr.h and the test entry points */

#define W 171u
#define H 107u
#define NA 6u  /* triangles with normals */
#define NB 5u  /* triangles without */
#define NT (NA + NB)

static float va[NA * 3][4], vb[NB * 3][4], uvs[NA * 3][2], na[NA * 3][3];
static uint32_t idx[NA * 3], vis[NA];
static rxr_batch3d batches[2];
static uint8_t px1[W * H * 4], px0[W * H * 4];
static uint32_t hs[NT][24], hh[NT][20], ds[NT][24], dh[NT][20];

static void triangles(float (*v)[4], uint32_t n, float x0, float y0, float z) {
    for (uint32_t t = 0; t < n; ++t) {
        const float x = x0 + 24.0f * (float)t, y = y0 + 7.0f * (float)t;
        const float p[3][2] = {{x, y}, {x + 37.0f, y + 5.0f}, {x + 9.0f, y + 41.0f}};
        for (int k = 0; k < 3; ++k) {
            v[3 * t + k][0] = p[k][0];
            v[3 * t + k][1] = p[k][1];
            v[3 * t + k][2] = z + 0.01f * (float)t;
            v[3 * t + k][3] = 1.0f + 0.25f * (float)k;
        }
    }
}

static void batch(rxr_batch3d *b, float (*v)[4], const float *normals, uint32_t nt, uint8_t r) {
    memset(b, 0, sizeof *b);
    b->projected_vertices = &v[0][0];
    b->clipped_uvs = &uvs[0][0];
    b->clipped_normals = normals;
    b->clipped_indices = idx;
    b->edge_visible = vis;
    b->cull_mode = RXR_CULL_OFF;
    b->n_vertices = nt * 3;
    b->n_triangles = nt;
    b->has_bounding_box = 1;
    b->bounding_box[0] = 0.0f; b->bounding_box[1] = 0.0f; b->bounding_box[2] = (float)W; b->bounding_box[3] = (float)H;
    b->source.kind = RXR_SOURCE_PIXEL;
    b->source.pixel[0] = r; b->source.pixel[1] = 90; b->source.pixel[2] = 40; b->source.pixel[3] = 255;
    b->ambient_color[0] = b->ambient_color[1] = b->ambient_color[2] = 1.0f;
    b->shader = -1;
    b->list = RXR_LIST_STATIC;
    b->chunk = -1;
}

static void frame(rxr_frame *f, const rxr_batch3d *b, uint32_t n) {
    memset(f, 0, sizeof *f);
    f->abi_version = RXR_ABI_VERSION;
    f->width = W;
    f->height = H;
    f->tile_size = 40;
    float *m[4] = {f->inverse_view, f->inverse_projection, f->view, f->projection};
    for (int k = 0; k < 4; ++k) {
        memset(m[k], 0, 64);
        m[k][0] = m[k][5] = m[k][10] = m[k][15] = 1.0f;
    }
    f->scaled2 = 1.0f;
    f->flags = RXR_FLAG_D3_ACTIVE;
    f->batches3d = b;
    f->n_batches3d = n;
}

/* uploads first a frame whose second batch HAS normals (sevens), then the frame under test; renders it whole */
static int run(rxr_ctx *ctx, uint8_t *pixels, uint32_t expect_route, int *failures) {
    static float sevens[NB * 3][3];
    for (uint32_t k = 0; k < NB * 3; ++k) sevens[k][0] = sevens[k][1] = sevens[k][2] = 7.0f;
    rxr_frame f;
    batch(&batches[0], va, &na[0][0], NA, 200);
    batch(&batches[1], vb, &sevens[0][0], NB, 60);
    frame(&f, batches, 2);
    int rc = rxr_upload_frame(ctx, &f);
    batch(&batches[1], vb, NULL, NB, 60);
    if (rc == RXR_OK) rc = rxr_upload_frame(ctx, &f);
    if (rc != RXR_OK) {
        printf("  ^^^ FAILED: rxr_upload_frame: %s\n", rxr_last_error(ctx));
        ++*failures;
        return rc;
    }
    uint32_t n = 0;
    memset(hs, 0xA5, sizeof hs); memset(hh, 0xA5, sizeof hh); memset(ds, 0x5A, sizeof ds); memset(dh, 0x5A, sizeof dh);
    const int has = rxr_debug_setup_records(ctx, hs, hh, ds, dh, NT, &n);
    printf("records: rc=%d triangles %u (expected route %u)\n", has, n, expect_route);
    if (has != (expect_route == 1u ? 1 : 0) || n != NT) {
        printf("  ^^^ FAILED: host records %s\n", expect_route == 1u ? "missing" : "present");
        ++*failures;
    }
    if (has == 1 && (memcmp(hs, ds, sizeof hs) != 0 || memcmp(hh, dh, sizeof hh) != 0)) {
        printf("  ^^^ FAILED: the host-made records differ from k_setup3d's\n");
        ++*failures;
    }
    /* TriShade words 9 .. 17 are the three normals: the first batch's are not zero, the second batch's are -- on the device as well */
    int with = 0, without = 0;
    for (uint32_t t = 0; t < NT; ++t)
        for (int k = 9; k < 18; ++k) {
            if (t < NA) with += dh[t][k] != 0u;
            else without += dh[t][k] != 0u;
        }
    if (with != (int)NA * 9 || without != 0) {
        printf("  ^^^ FAILED: normals in the records: %d non-zero words with normals (of %u), %d without (of 0)\n", with, NA * 9, without);
        ++*failures;
    }
    /* vertex 1 of triangle 1 has w = 0: TriShade.iw1, .u1w, .v1w (words 1, 4, 7) are +inf on the device and, where they exist, on the host */
    const uint32_t inf = 0x7F800000u;
    if (dh[1][1] != inf || dh[1][4] != inf || dh[1][7] != inf || (has == 1 && (hh[1][1] != inf || hh[1][4] != inf || hh[1][7] != inf))) {
        printf("  ^^^ FAILED: 1 / w and uv / w of the vertex with w = 0: device %08x %08x %08x host %08x %08x %08x\n", dh[1][1], dh[1][4], dh[1][7], hh[1][1], hh[1][4], hh[1][7]);
        ++*failures;
    }
    rc = rxr_render_rows(ctx, 0, H);
    if (rc == RXR_OK) rc = rxr_synchronize(ctx);
    const uint32_t route = rxr_debug_last_setup_route(ctx);
    if (rc == RXR_OK) rc = rxr_download_rows(ctx, pixels, 0, H);
    size_t drawn = 0;
    for (uint32_t k = 0; k < W * H; ++k) drawn += pixels[4 * k + 3] == 255 && (pixels[4 * k] | pixels[4 * k + 1] | pixels[4 * k + 2]);
    printf("frame: rc=%d set-up route %u, pixels drawn %zu\n", rc, route, drawn);
    if (rc != RXR_OK || route != expect_route || drawn < 2000) {
        printf("  ^^^ FAILED: the frame must render through route %u and show its triangles (%s)\n", expect_route, rxr_last_error(ctx));
        ++*failures;
    }
    return rc;
}

int main(void) {
    triangles(va, NA, 4.0f, 3.0f, 0.5f);
    triangles(vb, NB, 20.0f, 30.0f, 0.3f);
    va[4][3] = 0.0f;   /* vertex 1 of triangle 1 on the eye plane; its uv (0.4, 0.72) is not zero, so uv / w is inf and not NaN */
    for (uint32_t k = 0; k < NA * 3; ++k) {
        idx[k] = k;
        uvs[k][0] = 0.1f * (float)k;
        uvs[k][1] = 1.0f - 0.07f * (float)k;
        na[k][0] = 0.25f + (float)k; na[k][1] = -1.5f; na[k][2] = 1.0f;
    }
    for (uint32_t t = 0; t < NA; ++t) vis[t] = 1;
    rxr_ctx *with_records = NULL, *with_launch = NULL;
    setenv("RXR_HOST_SETUP", "1", 1);
    int rc1 = rxr_create(&with_records, 0);
    setenv("RXR_HOST_SETUP", "0", 1);
    int rc0 = rxr_create(&with_launch, 0);
    if (rc1 != RXR_OK || rc0 != RXR_OK) {
        printf("rxr_create failed\n");
        return 2;
    }
    int failures = 0;
    run(with_records, px1, 1u, &failures);
    run(with_launch, px0, 2u, &failures);
    if (memcmp(px1, px0, sizeof px1) != 0) {
        printf("  ^^^ FAILED: the frame from the host-made records differs from the frame behind k_setup3d\n");
        ++failures;
    }
    rxr_destroy(with_launch);
    rxr_destroy(with_records);
    printf("ok (%d failures)\n", failures);
    return failures ? 1 : 0;
}
