/* A C ABI caller whose batch box does not enclose its triangle, on a machine WITH a GPU.  One host-projected sparse frame: a triangle
 * that reaches x = 325, handed over with a bounding box that ends at x = 318 (ordinary coordinates: not a risky box, no NaN; small enough
 * for the bin lists, not the list of large triangles), and a batch of 160 small triangles lower down so that the frame is binned.  With tile size 16 the reference draws the first batch in the tile
 * columns left of x = 320 only, so the row spans of its rows end there -- and the triangle's own pixel box reaches the column behind.
 * After the frame, rxr_debug_scratch must find every word the next launch assumes zero at zero; then a dense frame on the same context
 * must equal the same dense frame on a fresh context byte for byte.  Run with RXR_CONTENT_MIN_TILES=0 (row spans on a small frame) by
 * tests/test_gpu_abi_sparse_box.py (gcc -std=c11 -Wall -Werror). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../rusterix_amd/csrc/rxr_debug.h" /* rxr.h and the test entry points */

#define W 480u
#define H 480u
#define NX 16u
#define NY 10u
#define NS (NX * NY)

static float big_v[3][4] = {{290.0f, 190.0f, 0.5f, 1.0f}, {325.0f, 200.0f, 0.5f, 1.0f}, {290.0f, 210.0f, 0.5f, 1.0f}};
static uint32_t big_i[3] = {0, 1, 2};
static float small_v[NS * 3][4];
static uint32_t small_i[NS * 3];
static float dense_v[4][4] = {{0.0f, 0.0f, 0.5f, 1.0f}, {480.0f, 0.0f, 0.5f, 1.0f}, {480.0f, 480.0f, 0.5f, 1.0f}, {0.0f, 480.0f, 0.5f, 1.0f}};
static uint32_t dense_i[6] = {0, 1, 2, 0, 2, 3};
static float uvs[NS * 3][2];
static float normals[NS * 3][3];   /* (0, 0, 1): a batch without normals shades to NaN -> 0 as in the reference */
static uint32_t vis[NS];
static rxr_batch3d batches[3];
static uint8_t pixels[W * H * 4], dense_a[W * H * 4], dense_b[W * H * 4];

static void batch(rxr_batch3d *b, float (*v)[4], uint32_t nv, const uint32_t *ix, uint32_t nt, float x, float y, float w, float h, uint8_t r) {
    memset(b, 0, sizeof *b);
    b->projected_vertices = &v[0][0];
    b->clipped_uvs = &uvs[0][0];
    b->clipped_normals = &normals[0][0];
    b->clipped_indices = ix;
    b->edge_visible = vis;
    b->cull_mode = RXR_CULL_OFF;
    b->n_vertices = nv;
    b->n_triangles = nt;
    b->has_bounding_box = 1;
    b->bounding_box[0] = x; b->bounding_box[1] = y; b->bounding_box[2] = w; b->bounding_box[3] = h;
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
    f->tile_size = 16;
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

/* the dense frame: a full-screen quad and the small triangles spread over most of the frame (binned, no row spans) */
static int render_dense(rxr_ctx *ctx, uint8_t *out) {
    static float moved[NS * 3][4];
    for (uint32_t k = 0; k < NS * 3; ++k) {
        moved[k][0] = small_v[k][0] * 1.6f - 60.0f;
        moved[k][1] = small_v[k][1] * 4.0f - 1400.0f;
        moved[k][2] = 0.25f;
        moved[k][3] = 1.0f;
    }
    rxr_batch3d b[2];
    batch(&b[0], dense_v, 4, dense_i, 2, 0.0f, 0.0f, 480.0f, 480.0f, 30);
    batch(&b[1], moved, NS * 3, small_i, NS, -60.0f, -1400.0f, 2000.0f, 2000.0f, 220);
    rxr_frame f;
    frame(&f, b, 2);
    return rxr_rasterize(ctx, &f, out);
}

int main(void) {
    for (uint32_t j = 0; j < NY; ++j)
        for (uint32_t i = 0; i < NX; ++i) {
            const uint32_t t = j * NX + i;
            const float x = 40.0f + 15.0f * (float)i, y = 350.0f + 9.0f * (float)j;
            const float p[3][2] = {{x, y}, {x + 7.0f, y}, {x, y + 7.0f}};
            for (int k = 0; k < 3; ++k) {
                small_v[3 * t + k][0] = p[k][0];
                small_v[3 * t + k][1] = p[k][1];
                small_v[3 * t + k][2] = 0.5f;
                small_v[3 * t + k][3] = 1.0f;
                small_i[3 * t + k] = 3 * t + k;
                normals[3 * t + k][2] = 1.0f;
            }
            vis[t] = 1;
        }
    rxr_ctx *ctx = NULL, *fresh = NULL;
    if (rxr_create(&ctx, 0) != RXR_OK || rxr_create(&fresh, 0) != RXR_OK) {
        printf("rxr_create failed\n");
        return 2;
    }
    int failures = 0;
    /* the box ends at x = 318 (290 + 28); the triangle reaches 325 */
    batch(&batches[0], big_v, 3, big_i, 1, 290.0f, 190.0f, 28.0f, 20.0f, 200);
    batch(&batches[1], small_v, NS * 3, small_i, NS, 40.0f, 350.0f, 232.0f, 88.0f, 60);
    rxr_frame f;
    frame(&f, batches, 2);
    int rc = rxr_rasterize(ctx, &f, pixels);
    uint32_t info[4] = {0}, dirt[4] = {0};
    rxr_debug_content(ctx, info);
    printf("sparse frame: rc=%d content rows %u..%u, row spans %u\n", rc, info[1], info[2], info[3]);
    if (rc != RXR_OK || info[3] != 1u) {
        printf("  ^^^ FAILED: the sparse frame must render with row spans (%s)\n", rxr_last_error(ctx));
        ++failures;
    }
    /* pixel (312, 200) is inside the triangle and the box: drawn; (320, 200) lies outside the reference's tiles: the miss colour */
    const uint8_t *in = &pixels[(200u * W + 312u) * 4u], *out = &pixels[(200u * W + 320u) * 4u];
    printf("pixel inside %u,%u,%u,%u  behind the box %u,%u,%u,%u\n", in[0], in[1], in[2], in[3], out[0], out[1], out[2], out[3]);
    if (in[3] != 255 || !(in[0] | in[1] | in[2]) || out[0] != 0 || out[1] != 0 || out[2] != 0 || out[3] != 255) {
        printf("  ^^^ FAILED: the reference draws the batch left of x = 320 only\n");
        ++failures;
    }
    rc = rxr_debug_scratch(ctx, dirt);
    printf("scratch after the sparse frame: rc=%d non-zero words %u (first: buffer %u word %u = %u)\n", rc, dirt[0], dirt[1], dirt[2], dirt[3]);
    if (rc != 0 || dirt[0] != 0) {
        printf("  ^^^ FAILED: words the next launch assumes zero are not\n");
        ++failures;
    }
    int ra = render_dense(ctx, dense_a), rb = render_dense(fresh, dense_b);
    rxr_debug_scratch(ctx, dirt);
    const int same = memcmp(dense_a, dense_b, sizeof dense_a) == 0;
    size_t drawn = 0;
    for (uint32_t k = 0; k < W * H; ++k) drawn += dense_a[4 * k + 3] == 255 && (dense_a[4 * k] | dense_a[4 * k + 1] | dense_a[4 * k + 2]);
    printf("dense frame: rc=%d / %d, equal to a fresh context's: %d, scratch words %u, pixels drawn %zu\n", ra, rb, same, dirt[0], drawn);
    if (ra != RXR_OK || rb != RXR_OK || !same || dirt[0] != 0 || drawn < (size_t)W * H * 9u / 10u) {
        printf("  ^^^ FAILED: the dense frame on the used context must equal the fresh context's\n");
        ++failures;
    }
    rxr_destroy(fresh);
    rxr_destroy(ctx);
    printf("ok (%d failures)\n", failures);
    return failures ? 1 : 0;
}
