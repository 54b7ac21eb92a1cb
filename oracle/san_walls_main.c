/*
 * san_walls_main.c — a stand-alone driver of the oracle's walled path for AddressSanitizer + UndefinedBehaviorSanitizer.
 *
 * TEST INFRASTRUCTURE ONLY.  `make -C oracle san-walls` compiles this file TOGETHER with rcw_oracle.c (it includes it: one
 * translation unit, so the file-local functions are checked too) under -fsanitize=address,undefined, once per world-unit width, and
 * runs both programs on the CPU.  Each drives orc_set_walls (all agents, masked, per-agent layouts, every refusal), resets, a masked
 * and an unmasked rollout under auto_reset with a top view, on maps with interior walls — a 5 x 7 map whose 2-bit fields run across
 * the tile map's word boundaries, a map without a free tile for the goal redraw's cap — and exits 0 if nothing was reported and the
 * invariants below hold.  tests/test_oracle_walls.py builds and runs it.
 */
#include <stdio.h>

#include "rcw_oracle.c"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "san_walls_main: %s failed (line %d)\n", #x, __LINE__); return 1; } } while (0)

static void ring(uint8_t* w, int H, int W)
{
    memset(w, 0, (size_t)H * W);
    for (int i = 0; i < H; ++i) { w[i] = 1; w[i + H * (W - 1)] = 1; }
    for (int j = 0; j < W; ++j) { w[H * j] = 1; w[(H - 1) + H * j] = 1; }
}

static rcw_config config(int H, int W, int N, int Hc, int top)
{
    rcw_config c;
    memset(&c, 0, sizeof c);
    c.abi_version = RCW_ABI_VERSION;
    c.height_tile_map_tu = H; c.width_tile_map_tu = W; c.num_directions = 8; c.num_rays = N; c.height_camera_view_pu = Hc;
    c.pu_per_tu = 5; c.render_top_view = top;
    c.player_radius_wu = 0.3f; c.position_increment_wu = 0.25f; c.semi_field_of_view_wu = 2.0f / 3.0f; c.camera_height_tile_wu = 1.0f;
    c.player_radius_wu_f64 = 0.3; c.position_increment_wu_f64 = 0.25; c.semi_field_of_view_wu_f64 = 2.0 / 3.0; c.camera_height_tile_wu_f64 = 1.0;
    c.goal_reward = 1.0f; c.goal_reward_f64 = 1.0;
    c.floor_color = 0x00404040; c.ceiling_color = 0x00FFFFFF; c.wall_dim_1_color = 0x00808080; c.wall_dim_2_color = 0x00C0C0C0;
    c.goal_dim_1_color = 0x00800000; c.goal_dim_2_color = 0x00C00000;
    c.auto_reset = 1; c.world_unit_bits = (int)(8 * sizeof(real));
    return c;
}

/* every agent stands on a free tile that is not its goal, the goal is on a free interior tile */
static int state_is_valid(orc_batch* b)
{
    const int H = b->H, W = b->W;
    for (int a = 0; a < b->B; ++a) {
        const uint8_t* wm = b->wall + (size_t)H * W * a;
        const int gi = b->goal[2 * a], gj = b->goal[2 * a + 1];
        const int pi = (int)R_FLOOR(b->pos[2 * a]) + 1, pj = (int)R_FLOOR(b->pos[2 * a + 1]) + 1;
        if (gi < 2 || gi > H - 1 || gj < 2 || gj > W - 1 || wm[(gi - 1) + H * (gj - 1)]) return 0;
        if (pi < 2 || pi > H - 1 || pj < 2 || pj > W - 1 || wm[(pi - 1) + H * (pj - 1)]) return 0;
        if (b->status[a] != 0) return 0;
    }
    return 1;
}

int main(void)
{
    enum { H = 5, W = 7, B = 9, N = 33, Hc = 24 };
    rcw_config c = config(H, W, N, Hc, 1);
    orc_batch* b = NULL;
    CHECK(orc_create(&c, B, 4, 1, &b) == RCW_OK);

    /* three layouts: the ring | two pillars | a bar with a door */
    uint8_t walls[3 * H * W];
    for (int m = 0; m < 3; ++m) ring(walls + m * H * W, H, W);
    walls[1 * H * W + 2 + H * 2] = 1; walls[1 * H * W + 2 + H * 4] = 7;       /* (any non-zero byte is a wall) */
    for (int i = 1; i < H - 1; ++i) walls[2 * H * W + i + H * 3] = 1;
    walls[2 * H * W + 2 + H * 3] = 0;
    int32_t index[B]; uint8_t mask[B], actions[B], moved[B];
    for (int a = 0; a < B; ++a) { index[a] = a % 3; mask[a] = (uint8_t)(a % 2); }

    CHECK(orc_set_walls(b, walls, 3, index, NULL) == RCW_OK);
    CHECK(state_is_valid(b));
    for (int a = 0; a < B; ++a) CHECK(b->episode[a] == 2);
    uint64_t chunks[B * 2];
    CHECK(orc_num_chunks(b) == 2);
    orc_tile_map_chunks(b, chunks);

    /* the refusals: each leaves the batch as it was */
    uint8_t bad[3 * H * W];
    memcpy(bad, walls, sizeof bad); bad[2 * H * W + 0 + H * 3] = 0;           /* a ring tile of a layout nobody need take */
    int32_t worse[B]; memcpy(worse, index, sizeof worse); worse[4] = 3;
    uint8_t full[H * W]; memset(full, 1, sizeof full); full[2 + H * 2] = 0;  /* one free interior tile */
    CHECK(orc_set_walls(b, NULL, 3, index, NULL) == RCW_ERR_INVALID_ARGUMENT);
    CHECK(orc_set_walls(b, walls, 0, index, NULL) == RCW_ERR_INVALID_ARGUMENT);
    CHECK(orc_set_walls(b, walls, 3, NULL, NULL) == RCW_ERR_INVALID_ARGUMENT);
    CHECK(orc_set_walls(b, walls, 3, worse, NULL) == RCW_ERR_INVALID_ARGUMENT);
    CHECK(orc_set_walls(b, bad, 3, index, NULL) == RCW_ERR_INVALID_ARGUMENT);
    CHECK(orc_set_walls(b, full, 1, NULL, NULL) == RCW_ERR_INVALID_ARGUMENT);
    uint64_t again[B * 2];
    orc_tile_map_chunks(b, again);
    CHECK(memcmp(chunks, again, sizeof chunks) == 0);
    for (int a = 0; a < B; ++a) CHECK(b->episode[a] == 2);
    worse[4] = 1; worse[3] = 99; mask[3] = 0;                                  /* (a masked-out agent's entry is not read) */
    CHECK(orc_set_walls(b, walls, 3, worse, mask) == RCW_OK);
    for (int a = 0; a < B; ++a) CHECK(b->episode[a] == 2u + mask[a]);
    CHECK(state_is_valid(b));

    /* a rollout: forward-heavy actions from a small generator, every third step a masked one, resets in between */
    uint64_t s = 12345;
    for (int t = 0; t < 200; ++t) {
        for (int a = 0; a < B; ++a) {
            s = orc_mix64(s + 1);
            const int r = (int)(s % 6);
            actions[a] = (uint8_t)(r < 3 ? 1 : r - 1);
            moved[a] = (uint8_t)((s >> 8) & 1);
        }
        if (t % 3 == 2) {
            for (int a = 0; a < B; ++a) if (!moved[a]) actions[a] = 0;       /* (not read) */
            CHECK(orc_step_masked(b, actions, moved) == RCW_OK);
        } else if (t % 7 == 3) {
            actions[2] = 9;
            CHECK(orc_step(b, actions) == RCW_ERR_INVALID_ACTION);
            CHECK(orc_step_lenient_masked(b, actions, t % 2 ? moved : NULL) == RCW_OK);
            orc_clear_status(b);
        } else {
            CHECK(orc_step(b, actions) == RCW_OK);
        }
        if (t == 60) CHECK(orc_reset(b, mask, 77) == RCW_OK);
        if (t == 120) CHECK(orc_set_walls(b, walls + 2 * H * W, 1, NULL, mask) == RCW_OK);
        CHECK(state_is_valid(b));
    }
    uint64_t redraws = 0, blocked = 0, episodes = 0;
    for (int a = 0; a < B; ++a) { redraws += b->goal_redraws[a]; blocked += b->blocked_inner[a]; episodes += b->episode[a]; }
    CHECK(redraws > 0 && blocked > 0 && episodes > 3u * B);
    orc_destroy(b);

    /* B layouts with a NULL index, and a map whose interior holds two free tiles that the goal pair (2..H-1 x 2..W-1) can reach */
    enum { H2 = 9, W2 = 9, B2 = 2 };
    c = config(H2, W2, 16, 16, 0);
    CHECK(orc_create(&c, B2, 1, 1, &b) == RCW_OK);
    uint8_t two[B2 * H2 * W2];
    memset(two, 1, sizeof two);
    two[3 + H2 * 3] = two[4 + H2 * 3] = 0;
    ring(two + H2 * W2, H2, W2); two[H2 * W2 + 4 + H2 * 4] = 1;
    CHECK(orc_set_walls(b, two, B2, NULL, NULL) == RCW_OK);
    CHECK(state_is_valid(b));
    CHECK(b->goal_redraws[0] > 0);
    for (int t = 0; t < 40; ++t) {
        for (int a = 0; a < B2; ++a) actions[a] = (uint8_t)(1 + (t + a) % 4);
        CHECK(orc_step(b, actions) == RCW_OK);
    }
    orc_destroy(b);
    printf("san_walls_main: clean (T = Float%d)\n", (int)(8 * sizeof(real)));
    return 0;
}
