/* oracle_hit_main.c — a stand-alone program over oracle/oracle.c's caller-ray entries (orc_world_hit,
 * orc_scene_hit), for tests/test_oracle_hits.py: compiled together with oracle.c under ASan and UBSan
 * and run directly (nothing is preloaded), and once more, uninstrumented, against liboracle.so; the
 * two must print the same lines.
 *
 * It builds a small nested world (spheres, a moving sphere, a translated and rotated box, a medium
 * under an instance, an instanced BVH of spheres, a medium bounded by a BVH) and the built-in scene 7
 * over a synthetic 8 x 4 image, runs both entries on a few hundred seeded rays with the three kinds of
 * interval (n = 0 and a batch that can only miss among them) and prints a checksum per batch. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../oracle/oracle.h"

static uint64_t lcg_state = 0x9E3779B97F4A7C15ull;
static double uniform(double a, double b)
{
    lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull;
    return a + (b - a) * ((double)(lcg_state >> 11) * (1.0 / 9007199254740992.0));
}

/* n rays from a box of half-width `extent` around `centre`, aimed into it, unnormalised */
static orc_ray* make_rays(int n, const double centre[3], double extent)
{
    orc_ray* rays = (orc_ray*)malloc((size_t)(n > 0 ? n : 1) * sizeof(orc_ray));
    for (int i = 0; i < n; ++i) {
        orc_ray* r = &rays[i];
        double len = uniform(0.4, 2.5), norm = 0.0, d[3];
        for (int a = 0; a < 3; ++a) {
            r->o[a] = centre[a] + uniform(-extent, extent);
            d[a] = centre[a] + uniform(-0.5 * extent, 0.5 * extent) - r->o[a];
            norm += d[a] * d[a];
        }
        norm = sqrt(norm);
        for (int a = 0; a < 3; ++a) r->d[a] = norm > 0.0 ? d[a] / norm * len : (a == 0 ? len : 0.0);
        r->time = uniform(0.0, 1.0);
        r->t_min = 0.001;
        r->t_max = INFINITY;
        if (i % 3 == 1) r->t_min = -uniform(0.5, 6.0) * extent;
        if (i % 3 == 2) r->t_max = uniform(0.5, 6.0) * extent;
        r->key_pixel = (uint32_t)uniform(0.0, 1048576.0);
        r->key_sample = (uint32_t)uniform(0.0, 64.0);
    }
    return rays;
}

static void report(const char* what, int n, const orc_hit* out)
{
    double cs = 0.0;
    int hits = 0, fronts = 0;
    for (int i = 0; i < n; ++i) {
        const orc_hit* h = &out[i];
        hits += h->hit;
        fronts += h->front_face;
        if (!h->hit) {
            if (!(isinf(h->t) && h->t > 0.0) || h->mat != 0 || h->top != 0 || h->p[0] != 0.0 || h->n[0] != 0.0 || h->albedo[0] != 0.0) {
                printf("%s: ray %d: a miss is not t = inf and zeros\n", what, i);
                exit(1);
            }
            continue;
        }
        cs += h->t + 2.0 * h->p[0] + 3.0 * h->p[1] + 5.0 * h->p[2] + 7.0 * h->n[0] + 11.0 * h->n[1] + 13.0 * h->n[2] +
              17.0 * h->albedo[0] + 19.0 * h->albedo[1] + 23.0 * h->albedo[2] + 29.0 * h->mat + 31.0 * h->top;
    }
    printf("%s: n %d hits %d front %d checksum %.17g\n", what, n, hits, fronts, cs);
}

static int nested_world(orc_world** out)
{
    orc_world* w = NULL;
    if (orc_world_create(5, &w)) return -1;
    const double grey[3] = {0.73, 0.73, 0.73}, odd[3] = {0.9, 0.9, 0.9}, red[3] = {0.65, 0.05, 0.05}, zero[3] = {0, 0, 0};
    const double steel[3] = {0.8, 0.8, 0.9};
    int white = orc_world_material(w, 0, orc_world_texture(w, 0, grey, zero, 0.0), zero, 0.0, 0.0);
    int check = orc_world_material(w, 0, orc_world_texture(w, 1, red, odd, 0.0), zero, 0.0, 0.0);
    int noise = orc_world_material(w, 0, orc_world_texture(w, 2, zero, zero, 4.0), zero, 0.0, 0.0);
    int metal = orc_world_material(w, 1, 0, steel, 0.1, 0.0);
    int glass = orc_world_material(w, 2, 0, zero, 0.0, 1.5);
    int phase = orc_world_material(w, 4, orc_world_texture(w, 0, steel, zero, 0.0), zero, 0.0, 0.0);
    const double c_ground[3] = {0, -1000, 0}, c_glass[3] = {0, 1, 0}, c0[3] = {2.2, 0.5, 1.5}, c1[3] = {2.2, 1.0, 1.5};
    orc_world_push(w, orc_world_sphere(w, noise, c_ground, 1000.0));
    orc_world_push(w, orc_world_sphere(w, glass, c_glass, 1.0));
    orc_world_push(w, orc_world_sphere(w, glass, c_glass, -0.9));
    orc_world_push(w, orc_world_moving_sphere(w, metal, c0, c1, 1.0, 0.0, 0.5));
    const double mn[3] = {0, 0, 0}, mx[3] = {0.8, 1.6, 0.8}, off[3] = {-2.5, 0.0, 1.5};
    orc_world_push(w, orc_world_translate(w, orc_world_rotate_y(w, orc_world_box(w, mn, mx, check), 25.0), off));
    const double unit[3] = {1, 1, 1}, off2[3] = {-0.5, 0.0, -0.5}, off3[3] = {1.5, 0.0, -2.5};
    int smoke = orc_world_constant_medium(
        w, orc_world_translate(w, orc_world_rotate_y(w, orc_world_box(w, mn, unit, white), 15.0), off2), 1.5, phase);
    orc_world_push(w, orc_world_translate(w, orc_world_rotate_y(w, smoke, 40.0), off3));
    int balls[6], pair[2];
    for (int i = 0; i < 6; ++i) {
        const double c[3] = {0.4 * i, 0.25, 0.0};
        balls[i] = orc_world_sphere(w, white, c, 0.2);
    }
    const double off4[3] = {1.5, 0.0, 2.5};
    orc_world_push(w, orc_world_translate(w, orc_world_rotate_y(w, orc_world_bvh(w, balls, 6, 0.0, 1.0), 70.0), off4));
    const double p0[3] = {3.0, 0.6, -0.8}, p1[3] = {3.7, 0.6, -0.8};
    pair[0] = orc_world_sphere(w, white, p0, 0.6);
    pair[1] = orc_world_sphere(w, white, p1, 0.6);
    orc_world_push(w, orc_world_constant_medium(w, orc_world_bvh(w, pair, 2, 0.0, 1.0), 1.2, phase));
    if (white < 0 || check < 0 || noise < 0 || metal < 0 || glass < 0 || phase < 0 || smoke < 0) return -1;
    *out = w;
    return 0;
}

int main(void)
{
    enum { N = 300, N_MISS = 40 };
    orc_hit* out = (orc_hit*)malloc(N * sizeof(orc_hit));
    orc_world* w = NULL;
    if (nested_world(&w)) { printf("world construction failed\n"); return 1; }

    const double middle[3] = {0.0, 0.7, 0.0};
    orc_ray* rays = make_rays(N, middle, 4.0);
    for (uint32_t bounce = 0; bounce < 4; bounce += 3) {
        if (orc_world_hit(w, 5, bounce, N, rays, out)) return 1;
        report(bounce ? "world, bounce 3" : "world, bounce 0", N, out);
    }
    if (orc_world_hit(w, 5, 0, 0, NULL, NULL)) return 1;                 /* n = 0 */
    if (orc_world_hit(w, 5, 0, 0, rays, out)) return 1;
    const double above[3] = {0.0, 50.0, 0.0};                             /* rays that start above everything and go up */
    orc_ray* miss = make_rays(N_MISS, above, 4.0);
    for (int i = 0; i < N_MISS; ++i) {
        miss[i].d[1] = 1.0 + fabs(miss[i].d[1]);
        miss[i].t_min = 0.001;
    }
    if (orc_world_hit(w, 5, 0, N_MISS, miss, out)) return 1;
    report("world, misses only", N_MISS, out);
    free(miss);
    free(rays);
    orc_world_destroy(w);

    /* scene 7 (main.rs:173-243) over an 8 x 4 image */
    uint8_t image[8 * 4 * 3];
    for (int i = 0; i < 8 * 4 * 3; ++i) image[i] = (uint8_t)(37 * i + 11);
    const double room[3] = {278.0, 278.0, 200.0};
    rays = make_rays(N, room, 400.0);
    if (orc_scene_hit(7, 1, image, 8, 4, 5, 0, N, rays, out)) return 1;
    report("scene 7, bounce 0", N, out);
    if (orc_scene_hit(7, 1, image, 8, 4, 5, 3, N, rays, out)) return 1;
    report("scene 7, bounce 3", N, out);
    if (orc_scene_hit(7, 1, image, 8, 4, 5, 0, 0, NULL, NULL)) return 1;  /* n = 0 */
    const double outside[3] = {0.0, 20000.0, 0.0};                        /* beyond the 5,000 fog sphere, going away */
    miss = make_rays(N_MISS, outside, 100.0);
    for (int i = 0; i < N_MISS; ++i) {
        miss[i].d[1] = 1.0 + fabs(miss[i].d[1]);
        miss[i].t_min = 0.001;
    }
    if (orc_scene_hit(7, 1, image, 8, 4, 5, 0, N_MISS, miss, out)) return 1;
    report("scene 7, misses only", N_MISS, out);
    if (orc_scene_hit(7, 1, NULL, 0, 0, 5, 0, N, rays, out) != -2 || orc_scene_hit(9, 1, image, 8, 4, 5, 0, N, rays, out) != -1) {
        printf("bad arguments accepted\n");
        return 1;
    }
    free(miss);
    free(rays);
    free(out);
    return 0;
}
