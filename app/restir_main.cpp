/*
 * restir_main.cpp — headless C++ host of the hot path: the frame loop of the reference's
 * examples/10_restir_di/10_restir_di.cpp:23-416 without GLFW/OpenGL/Orochi/HIPRT, written
 * against the C-ABI only: include/restir_rt.h for everything the example's frame loop does; restir_rt_internal.h
 * supplies what its measurement switches add (--mirror / --shm stand-in transports, --cost-strips' rt_row_shaded,
 * the path tracers' ray counter).
 *
 *   restir_app [--obj scene.obj | --tris scene.tris] [--size W H] [--frames N]
 *              [--eye x y z] [--lookat x y z] [--temporal 0|1] [--spatial 0|1]
 *              [--shadowed 0|1] [--visreuse 0|1] [--accumulate 0|1] [--by-kernel]
 *              [--example 10|7|8|9|6|4] [--ppm out.ppm] [--png out.png] [--pfm out.pfm] [--rgba out.raw] [--dump-tris out.tris]
 *              [--ranks N [--mirror | --shm] [--bounds 0,a,b,...,H | --cost-strips]] [--threads N]
 *              [--move-lights dx dy dz] [--denoise N [--denoise-temporal]] [--orbit dx dy] [--unbiased] [--reproject] [--unbiased-temporal]
 *              [--move-tris first count dx dy dz] [--follow-motion] [--follow-lights] [--denoise-follow-motion]
 *              [--denoise-antilag [radius lo hi floor]]
 *              [--light-sampling uniform|power] [--light-grid CELLS CLUSTERS] [--indirect N]
 *
 * --example 4: BASELINE config #1 — the `kernelMain` of examples/04_ao/04_ao.cu:31-88 as a host C++ loop over the
 * image rows (cedec_2024_rt_amd/csrc/host_path.h: brute-force closest hit, 64 ambient-occlusion rays per pixel,
 * host libm), on --threads host threads (default: all). No GPU call is made: it runs on a machine without one.
 * Defaults then follow 04_ao.cpp (256x256 is the BASELINE size; camera (8,8,8) -> (0,0,0), common/misc.hpp:217-218);
 * --rgba writes the W*H RGBA8 bytes in the reference's storage order (what its pixel buffer holds).
 * --denoise N (--example 10, 7, 8, 9; one GPU): after every frame rt_denoise with N a-trous iterations (0..8) and the default
 * parameters; --ppm / --png / --rgba then write its tone-mapped image and --pfm its HDR image (RT_BUF_DENOISED).
 * --denoise-temporal (with --denoise N): rt_denoise_temporal (default alphas) in place of rt_denoise, one call per frame.
 * --unbiased (--example 10, one GPU): rt_spatial_unbiased, the spatial passes normalise by 1/Z; not with
 * --shadowed 1.
 * --indirect N (--example 10, one GPU): rt_indirect, every frame adds N = 1..32 bounces of path-traced indirect light (08_nee's depth
 * loop from depth 1, started at the G-buffer) between resolve and tone mapping.
 * --light-grid CELLS CLUSTERS (--example 10, one GPU): rt_light_grid, the candidates draw a cluster of lights from the table of their
 * surface point's grid cell (cluster power over squared distance) and a light from the cluster's alias table;
 * 1..32 cells per axis and 1..256 clusters, suggested 16 64; while it is given it decides over --light-sampling.
 * --light-sampling power (--example 10, also with --ranks): rt_light_sampling, the candidates pick their emissive triangle with a
 * probability proportional to area x luminance from an alias table; uniform: the reference's, default.
 * --reproject (--example 10, one GPU): rt_temporal_reprojection, after a camera move the temporal merge takes a pixel's history from the
 *     previous frame's pixel that saw the same surface point; meant for --orbit, a camera that stands still
 *     renders what it renders without the flag.
 * --unbiased-temporal (with --reproject): rt_temporal_unbiased, a temporal merge whose history comes from another pixel normalises by
 *     1/Z, at the price of at most one shadow ray from the history's origin; meant for --orbit dx dy
 *     --reproject, and with --unbiased for a frame whose every reuse step normalises by 1/Z. Not with --follow-motion.
 * --orbit dx dy (one GPU): before every frame from the second on, rt_camera_orbit(dx, dy) (a left-button drag); with
 * --accumulate 1 that frame starts a new accumulation, as the example clears on a camera update.
 * --move-lights dx dy dz (--example 10, also with --ranks): before every frame from the second on, the emissive triangles move
 * by (dx, dy, dz) and rt_scene_update refits the scene (the span from the lowest to the highest emissive index); the call's wall
 * time is printed per frame, and with --accumulate 1 the frame starts a new accumulation.
 * --move-tris first count dx dy dz (--example 10, also with --ranks): the general form of --move-lights, every triangle of
 *     [first, first + count) moves by (dx, dy, dz) before every frame from the second on (the same float add); not with --move-lights.
 * --follow-motion (with --reproject): rt_temporal_motion, the temporal merge of a pixel on a moved triangle takes the history of the
 *     previous frame's pixel that saw the point it was at; meant for --move-tris on non-emissive triangles.
 * --follow-lights (--example 10, one GPU; needs neither --reproject nor --follow-motion): rt_temporal_light_motion, for --move-lights and
 *     for --move-tris over emissive triangles: the light samples of the temporal history are carried along with the emitters they
 *     lie on at every update. Prints the re-based / located / moved / emptied totals at the end.
 * --denoise-follow-motion (with --denoise N --denoise-temporal): rt_denoise_temporal_motion, the denoiser's history of a pixel on a
 *     moved triangle is looked up from where its surface point was; meant for --move-tris. Each frame's
 *     denoise line then says whether the call followed.
 * --denoise-antilag [radius lo hi floor] (with --denoise N --denoise-temporal): rt_denoise_temporal_antilag, the temporal denoiser
 *     raises its blend factors where the current frame and the reprojected history disagree over a window;
 *     without the four numbers: the library's defaults. Each frame's denoise line then says whether the call was an adapted call.
 * --example 6: the same ambient occlusion ON THE GPU through rt_path_trace (examples/06_ao_hiprt/06_ao_hiprt.cu:35-91, the
 * same image as 04_ao's kernel). Defaults follow 06_ao_hiprt.cpp:79-80: 1920x1080, camera (8,8,8) -> (0,0,0), fovy pi/4.
 * --frames K times K launches after one warm-up (host clock around rt_sync) and prints ms per launch and Mray/s in the
 * reference's rays (W*H primary rays + 64 per hit pixel); --rgba / --ppm / --png as for --example 4.
 *
 * --ranks N: the multi-GPU frame loop: N processes, forked before anything touches a GPU,
 * rank r on device r, each rendering one row strip through the native strip driver (rt_mg_*: sparse
 * reservoir halos over RCCL send/recv with rank +-1). Strip heights: equal rows by default; --bounds gives the
 * edges explicitly (e.g. a cut measured by tools/strip_overhead.py, profiles/strip_cuts.json); --cost-strips weights
 * rows by their shaded pixels (round 2's model; measured worse than equal rows at 3840x2160, docs/MEASUREMENT_LOG_r01_r03.md). --pfm then receives every rank's rows (one file, written in
 * place). --mirror: all ranks on device 0 with the MIRROR transport (1-GPU boxes; timing/launch smoke
 * run, the image is not a frame). --shm: all ranks on device 0 with the host-staged shared-memory transport
 * (exact image, slow).
 * --example 7|8|9 runs the `path_trace` kernel of examples/07_pt, 08_nee or 09_ris instead of the
 * ReSTIR DI frame (one sample per pixel and frame; use --accumulate 1 to average frames).
 * Keys 1,2,3,4,A of the example (10_restir_di.cpp:143-174) are the --temporal/--spatial/
 * --shadowed/--visreuse/--accumulate flags; key S (screenshot, an RGB PNG written top row first,
 * common/misc.hpp:226-245) is --png (or --ppm). `--tris` reads a raw
 * array of 60-byte Triangle records (cedec_2024_rt_amd.scenes can write one); `--obj` uses the
 * OBJ/MTL subset the reference's loader consumes (common/loader.hpp:11-66: positions, faces as
 * triangle fans, per-face usemtl -> Kd/Ke).
 */
#include <atomic>
#include <cctype>
#include <cmath>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/wait.h>
#include <unistd.h>

#include "../include/restir_rt.h"
#include "../include/restir_rt_internal.h" /* --mirror, --shm, --cost-strips, rt_path_trace_rays */
#include "../cedec_2024_rt_amd/csrc/host_path.h"

/* RGB8 PNG, top row first, as saveScreenshot writes it (common/misc.hpp:226-245 via stbi_write_png);
 * the deflate stream uses stored blocks only (no compression: no zlib dependency). */
static void write_png(const char* path, int W, int H, const uint8_t* rgb /* W*H*3, top-down */)
{
    static uint32_t crc_table[256];
    if (!crc_table[1])
        for (uint32_t n = 0; n < 256; ++n)
        {
            uint32_t c = n;
            for (int k = 0; k < 8; ++k) c = (c & 1u) ? 0xedb88320u ^ (c >> 1) : c >> 1;
            crc_table[n] = c;
        }
    auto crc = [&](const std::vector<uint8_t>& d, size_t from) {
        uint32_t c = 0xffffffffu;
        for (size_t i = from; i < d.size(); ++i) c = crc_table[(c ^ d[i]) & 0xffu] ^ (c >> 8);
        return c ^ 0xffffffffu;
    };
    auto be32 = [](std::vector<uint8_t>& d, uint32_t v) { for (int s = 24; s >= 0; s -= 8) d.push_back((uint8_t)(v >> s)); };
    std::vector<uint8_t> raw; /* filter byte 0 + RGB per scanline */
    raw.reserve((size_t)H * (1 + 3 * (size_t)W));
    for (int y = 0; y < H; ++y)
    {
        raw.push_back(0);
        raw.insert(raw.end(), rgb + (size_t)y * W * 3, rgb + (size_t)(y + 1) * W * 3);
    }
    std::vector<uint8_t> z = {0x78, 0x01};
    uint32_t a = 1, b = 0; /* adler32 */
    for (size_t off = 0; off < raw.size() || off == 0; off += 65535)
    {
        const size_t n = raw.size() - off < 65535 ? raw.size() - off : 65535;
        z.push_back(off + n >= raw.size() ? 1 : 0);
        z.push_back((uint8_t)(n & 0xff)); z.push_back((uint8_t)(n >> 8));
        z.push_back((uint8_t)(~n & 0xff)); z.push_back((uint8_t)((~n >> 8) & 0xff));
        z.insert(z.end(), raw.begin() + (long)off, raw.begin() + (long)(off + n));
        for (size_t i = off; i < off + n; ++i) { a = (a + raw[i]) % 65521u; b = (b + a) % 65521u; }
        if (raw.empty()) break;
    }
    be32(z, (b << 16) | a);
    FILE* f = fopen(path, "wb");
    if (!f) { fprintf(stderr, "cannot write %s\n", path); exit(1); }
    const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    fwrite(sig, 1, 8, f);
    auto chunk = [&](const char* type, const std::vector<uint8_t>& payload) {
        std::vector<uint8_t> d;
        be32(d, (uint32_t)payload.size());
        d.insert(d.end(), type, type + 4);
        d.insert(d.end(), payload.begin(), payload.end());
        be32(d, crc(d, 4));
        fwrite(d.data(), 1, d.size(), f);
    };
    std::vector<uint8_t> ihdr;
    be32(ihdr, (uint32_t)W); be32(ihdr, (uint32_t)H);
    const uint8_t tail[5] = {8, 2, 0, 0, 0}; /* 8 bits, colour type 2 (RGB), deflate, no filter, no interlace */
    ihdr.insert(ihdr.end(), tail, tail + 5);
    chunk("IHDR", ihdr);
    chunk("IDAT", z);
    chunk("IEND", {});
    fclose(f);
}

/* the ambient-occlusion image (W*H RGBA8 in the reference's storage order, bottom row first) as --rgba / --ppm / --png ask */
static int write_ao_image(const std::vector<uint8_t>& px, int W, int H, const std::string& rgba, const std::string& ppm, const std::string& png)
{
    if (!rgba.empty())
    {
        FILE* f = fopen(rgba.c_str(), "wb");
        if (!f) { fprintf(stderr, "cannot write %s\n", rgba.c_str()); return 1; }
        fwrite(px.data(), 1, px.size(), f);
        fclose(f);
    }
    if (!ppm.empty())
    {
        FILE* f = fopen(ppm.c_str(), "wb");
        if (!f) { fprintf(stderr, "cannot write %s\n", ppm.c_str()); return 1; }
        fprintf(f, "P6\n%d %d\n255\n", W, H);
        for (int y = H - 1; y >= 0; --y)
            for (int x = 0; x < W; ++x) fwrite(&px[4 * ((size_t)y * W + x)], 1, 3, f);
        fclose(f);
    }
    if (!png.empty())
    {
        std::vector<uint8_t> rgb((size_t)W * H * 3);
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) memcpy(&rgb[3 * ((size_t)y * W + x)], &px[4 * ((size_t)(H - 1 - y) * W + x)], 3);
        write_png(png.c_str(), W, H, rgb.data());
    }
    return 0;
}

static void die(rt_ctx* c, const char* what, int rc)
{
    fprintf(stderr, "%s failed (%d): %s\n", what, rc, c ? rt_last_error(c) : "");
    exit(1);
}
#define CK(call)                                  \
    do                                            \
    {                                             \
        int _rc = (call);                         \
        if (_rc != RT_OK) die(ctx, #call, _rc);   \
    } while (0)

struct Mtl { float kd[3] = {0, 0, 0}, ke[3] = {0, 0, 0}; };

static std::map<std::string, Mtl> load_mtl(const std::string& path)
{
    std::map<std::string, Mtl> m;
    std::ifstream f(path);
    std::string line, cur;
    while (std::getline(f, line))
    {
        std::istringstream ss(line);
        std::string k;
        ss >> k;
        if (k == "newmtl") { ss >> cur; m[cur] = Mtl(); }
        else if (k == "Kd" && !cur.empty()) ss >> m[cur].kd[0] >> m[cur].kd[1] >> m[cur].kd[2];
        else if (k == "Ke" && !cur.empty()) ss >> m[cur].ke[0] >> m[cur].ke[1] >> m[cur].ke[2];
    }
    return m;
}

static std::vector<rt_triangle> load_obj(const std::string& path)
{
    std::vector<rt_triangle> out;
    std::ifstream f(path);
    if (!f) { fprintf(stderr, "cannot open %s\n", path.c_str()); exit(1); }
    const std::string dir = path.find('/') == std::string::npos ? "." : path.substr(0, path.rfind('/'));
    std::vector<float> v;
    std::map<std::string, Mtl> mats;
    Mtl cur;
    std::string line;
    while (std::getline(f, line))
    {
        std::istringstream ss(line);
        std::string k;
        ss >> k;
        if (k == "v") { float x, y, z; ss >> x >> y >> z; v.push_back(x); v.push_back(y); v.push_back(z); }
        else if (k == "mtllib") { std::string n; ss >> n; auto m = load_mtl(dir + "/" + n); mats.insert(m.begin(), m.end()); }
        else if (k == "usemtl") { std::string n; ss >> n; cur = mats.count(n) ? mats[n] : Mtl(); }
        else if (k == "f")
        {
            std::vector<int> idx;
            std::string w;
            while (ss >> w)
            {
                const int i = atoi(w.substr(0, w.find('/')).c_str());
                idx.push_back(i > 0 ? i - 1 : (int)(v.size() / 3) + i);
            }
            for (size_t t = 2; t < idx.size(); ++t) /* triangle fan, tiny_obj_loader.h:908-931 */
            {
                rt_triangle tri;
                const int id[3] = {idx[0], idx[t - 1], idx[t]};
                for (int a = 0; a < 3; ++a)
                    for (int c = 0; c < 3; ++c) tri.v[a][c] = v[3 * (size_t)id[a] + c];
                memcpy(tri.color, cur.kd, 12);
                memcpy(tri.emissive, cur.ke, 12);
                out.push_back(tri);
            }
        }
    }
    return out;
}

static std::vector<rt_triangle> load_tris(const std::string& path)
{
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) { fprintf(stderr, "cannot open %s\n", path.c_str()); exit(1); }
    const size_t bytes = (size_t)f.tellg();
    std::vector<rt_triangle> t(bytes / sizeof(rt_triangle));
    f.seekg(0);
    f.read((char*)t.data(), (std::streamsize)(t.size() * sizeof(rt_triangle)));
    return t;
}

/* ---- --move-lights dx dy dz (--example 10): before frame f >= 2 every emissive triangle moves by (dx, dy, dz) from where it
 * was (one float add per coordinate, as scenes.move_triangles) and rt_scene_update refits the scene over the span from the
 * lowest to the highest emissive index; with --accumulate 1 that frame clears the accumulation (as after a camera move). After
 * the last update the app prints rt_bvh_cost's now / at_build ---- */
struct LightMove
{
    bool on = false;
    float d[3] = {0.0f, 0.0f, 0.0f};
    uint32_t first = 0, count = 0;
    bool all = false; /* --move-tris: every triangle of the span, emissive or not */
};
static void light_span(const std::vector<rt_triangle>& tris, LightMove& mv)
{
    uint32_t lo = 0xffffffffu, hi = 0u;
    for (size_t i = 0; i < tris.size(); ++i)
        if (tris[i].emissive[0] > 0.0f || tris[i].emissive[1] > 0.0f || tris[i].emissive[2] > 0.0f)
        {
            lo = lo < (uint32_t)i ? lo : (uint32_t)i;
            hi = (uint32_t)i;
        }
    mv.first = lo == 0xffffffffu ? 0u : lo;
    mv.count = lo == 0xffffffffu ? 0u : hi - lo + 1u;
}
/* moves the lights of the span and updates the context; returns the call's wall time in ms */
static double move_lights(rt_ctx* ctx, std::vector<rt_triangle>& tris, const LightMove& mv)
{
    for (uint32_t i = mv.first; i < mv.first + mv.count; ++i)
    {
        rt_triangle& t = tris[i];
        if (!mv.all && !(t.emissive[0] > 0.0f || t.emissive[1] > 0.0f || t.emissive[2] > 0.0f)) continue;
        for (int k = 0; k < 3; ++k)
            for (int a = 0; a < 3; ++a) t.v[k][a] = t.v[k][a] + mv.d[a];
    }
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = rt_scene_update(ctx, tris.data() + mv.first, mv.first, mv.count);
    if (rc != RT_OK) die(ctx, "rt_scene_update", rc);
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}
/* after the last update: what the refits have cost the tree (rt_bvh_cost: now / at build; rebuilding is the caller's decision) */
static void print_bvh_cost(rt_ctx* ctx)
{
    double now = 0.0, at_build = 0.0;
    const int rc = rt_bvh_cost(ctx, &now, &at_build);
    if (rc != RT_OK) die(ctx, "rt_bvh_cost", rc);
    printf("bvh cost now / at build: %.4f / %.4f = %.3f\n", now, at_build, at_build > 0.0 ? now / at_build : 1.0);
}

/* ---- --ranks N: one process per GPU over the native strip driver ---- */
struct Shared /* anonymous shared mapping made by the parent before fork */
{
    std::atomic<int> arrived[8];
    char uid[128];
    std::atomic<int> uid_ready;
    double ms_per_frame[64];
    unsigned long long rays[64];
    uint32_t row_cost[1]; /* H entries */
};
static void shared_barrier(Shared* sh, int which, int ranks)
{
    sh->arrived[which].fetch_add(1);
    for (long spins = 0; sh->arrived[which].load() < ranks; ++spins)
    {
        if (spins > 1500000L) { fprintf(stderr, "a rank did not reach barrier %d within 300 s\n", which); _exit(3); }
        usleep(200);
    }
}
static int rank_main(int rank, int ranks, bool mirror, bool shm, bool equal_strips, const std::vector<int>& given_bounds, Shared* sh,
                     const std::vector<rt_triangle>& triangles, int W, int H, int frames, const float* eye, const float* lookat, const rt_options& opt, int light_mode,
                     const std::string& pfm, const LightMove& mv)
{
    std::vector<rt_triangle> moving = mv.on ? triangles : std::vector<rt_triangle>();
    const float up[3] = {0, 1, 0};
    const int halo = 87, device = (mirror || shm) ? 0 : rank;
    if (rank == 0 && shm) snprintf(sh->uid, sizeof(sh->uid), "rtmg_app_%d_%llx", (int)getppid(),
                                  (unsigned long long)std::chrono::steady_clock::now().time_since_epoch().count()); /* per-run nonce */
    if (rank == 0 && !mirror && !shm)
    {
        if (rt_mg_unique_id(sh->uid) != RT_OK) { fprintf(stderr, "rank 0: %s\n", rt_mg_load_error()); return 1; }
    }
    if (rank == 0) sh->uid_ready.store(1);
    while (!sh->uid_ready.load()) usleep(200);
    std::vector<int> bounds((size_t)ranks + 1);
    if (rt_mg_partition(H, ranks, halo, nullptr, bounds.data()) != RT_OK) { fprintf(stderr, "%d rows cannot be cut into %d strips of >= %d rows\n", H, ranks, halo); return 1; }
    if (!given_bounds.empty())
    {
        bool ok = (int)given_bounds.size() == ranks + 1 && given_bounds.front() == 0 && given_bounds.back() == H;
        for (int r = 0; ok && r < ranks; ++r) ok = given_bounds[(size_t)r + 1] - given_bounds[(size_t)r] >= halo;
        if (!ok) { fprintf(stderr, "--bounds: %d + 1 edges from 0 to %d, strips of >= %d rows\n", ranks, H, halo); return 1; }
        bounds = given_bounds;
    }
    rt_ctx* ctx = nullptr;
    auto make_ctx = [&]() -> int {
        int rc = rt_create(device, W, H, bounds[(size_t)rank], bounds[(size_t)rank + 1], halo, &ctx);
        if (rc != RT_OK) return rc;
        rc = rt_scene_set(ctx, triangles.data(), (uint32_t)triangles.size());
        if (rc == RT_OK) rc = rt_camera_lookat(ctx, eye, lookat, up, 3.14159265358979323846f / 4.0f);
        if (rc == RT_OK) rc = rt_options_set(ctx, &opt);
        if (rc == RT_OK) rc = rt_light_sampling(ctx, light_mode);
        return rc;
    };
    int rc = make_ctx();
    if (rc != RT_OK) die(ctx, "strip context", rc);
    if (!equal_strips && given_bounds.empty())
    {
        /* cost-weighted heights: shaded pixels per row from one raycast of the equal partition */
        CK(rt_raycast(ctx));
        CK(rt_row_shaded(ctx, sh->row_cost + bounds[(size_t)rank]));
        shared_barrier(sh, 0, ranks);
        std::vector<uint32_t> cost((size_t)H);
        for (int i = 0; i < H; ++i) cost[(size_t)i] = sh->row_cost[i] * 7u + (uint32_t)W;
        std::vector<int> nb((size_t)ranks + 1);
        if (rt_mg_partition(H, ranks, halo, cost.data(), nb.data()) == RT_OK && nb != bounds)
        {
            CK(rt_destroy(ctx));
            bounds = nb;
            rc = make_ctx();
            if (rc != RT_OK) die(ctx, "strip context", rc);
        }
    }
    rt_mg* mg = nullptr;
    rc = rt_mg_create(ctx, rank, ranks, bounds.data(), shm ? (int)RT_MG_TRANSPORT_SHM : (mirror ? (int)RT_MG_TRANSPORT_MIRROR : (int)RT_MG_TRANSPORT_RCCL),
                      mirror ? nullptr : sh->uid, 0, &mg);
    if (rc != RT_OK) { fprintf(stderr, "rank %d: rt_mg_create failed (%d): %s\n", rank, rc, mg ? rt_mg_last_error(mg) : ""); return 1; }
    CK(rt_clear(ctx));
    const int warm = frames > 4 ? 2 : 0;
    struct timespec t0, t1;
    for (int frame = 1; frame <= frames; ++frame)
    {
        if (frame == warm + 1) { CK(rt_sync(ctx)); shared_barrier(sh, 1, ranks); clock_gettime(CLOCK_MONOTONIC, &t0); }
        int clear = 0;
        if (mv.on && frame >= 2 && mv.count > 0)
        {
            const double ms = move_lights(ctx, moving, mv);
            if (rank == 0) printf("frame %d scene update: %.3f ms (%u triangles)\n", frame, ms, mv.count);
            if (rank == 0 && frame == frames) print_bvh_cost(ctx);
            clear = opt.accumulate ? 1 : 0;
        }
        rc = rt_mg_frame(mg, frame, clear);
        if (rc != RT_OK) { fprintf(stderr, "rank %d frame %d: %s\n", rank, frame, rt_mg_last_error(mg)); return 1; }
    }
    CK(rt_sync(ctx));
    clock_gettime(CLOCK_MONOTONIC, &t1);
    sh->ms_per_frame[rank] = ((double)(t1.tv_sec - t0.tv_sec) * 1e3 + (double)(t1.tv_nsec - t0.tv_nsec) * 1e-6) / (double)(frames - warm);
    uint64_t rays = 0, shaded = 0;
    CK(rt_ray_count(ctx, &rays, &shaded));
    sh->rays[rank] = rays;
    rt_mg_stats st;
    rt_mg_get_stats(mg, &st);
    printf("rank %d: rows [%d,%d) %.3f ms/frame, host %.0f us/frame, %llu cold frame(s), %.2f MB sent/frame\n", rank, bounds[(size_t)rank],
           bounds[(size_t)rank + 1], sh->ms_per_frame[rank], (double)st.host_ns / 1e3 / (double)st.frames, st.cold_frames,
           (double)st.bytes_sent / 1e6 / (double)st.frames);
    if (!pfm.empty())
    {
        int l0 = 0, ln = 0;
        CK(rt_local_rows(ctx, &l0, &ln));
        std::vector<float> acc((size_t)W * (size_t)ln * 4);
        CK(rt_download(ctx, RT_BUF_ACCUMULATION, acc.data(), acc.size() * 4));
        char hdr[64];
        const int hl = snprintf(hdr, sizeof(hdr), "PF\n%d %d\n-1.0\n", W, H);
        const int fd = open(pfm.c_str(), O_WRONLY);
        if (fd < 0) { fprintf(stderr, "cannot write %s\n", pfm.c_str()); return 1; }
        std::vector<float> rgb((size_t)W * 3);
        for (int row = bounds[(size_t)rank]; row < bounds[(size_t)rank + 1]; ++row)
        {
            const float* a = &acc[(size_t)(row - l0) * W * 4];
            for (int x = 0; x < W; ++x)
                for (int c = 0; c < 3; ++c) rgb[3 * (size_t)x + c] = a[4 * (size_t)x + c] / a[4 * (size_t)x + 3];
            if (pwrite(fd, rgb.data(), rgb.size() * 4, (off_t)hl + (off_t)row * W * 12) < 0) return 1;
        }
        close(fd);
    }
    shared_barrier(sh, 2, ranks);
    if (rank == 0)
    {
        double worst = 0.0;
        unsigned long long total = 0;
        for (int r = 0; r < ranks; ++r) { worst = sh->ms_per_frame[r] > worst ? sh->ms_per_frame[r] : worst; total += sh->rays[r]; }
        printf("%d ranks: %.3f ms/frame (slowest rank), %llu rays/frame, %.0f Mray/s\n", ranks, worst, total, (double)total / worst / 1e3);
    }
    rt_mg_destroy(mg);
    CK(rt_destroy(ctx));
    return 0;
}

int main(int argc, char** argv)
{
    setenv("GPU_MAX_HW_QUEUES", "8", 0); /* five streams side by side per rank: before the first HIP call */
    int W = 1920, H = 1080, frames = 8; /* 10_restir_di.cpp:26-27 */
    /* camera "blocks_restir.obj 1", 10_restir_di.cpp:188-189 */
    float eye[3] = {-0.579885f, 22.194597f, -6.567105f}, lookat[3] = {5.224952f, 20.847435f, 1.431192f};
    const float up[3] = {0, 1, 0};
    std::string obj, tris_path, ppm, png, pfm, dump, rgba;
    bool by_kernel = false, mirror = false, shm = false, equal_strips = true, size_set = false, cam_set = false;
    std::vector<int> given_bounds;
    int example = 10, ranks = 1, threads = 0, denoise = -1;
    bool denoise_temporal = false, orbit = false, unbiased = false, reproject = false, unbiased_temporal = false, follow_motion = false, follow_lights = false, move_lights_given = false, denoise_follow = false;
    bool denoise_antilag = false, antilag_given = false;
    rt_denoise_antilag_params antilag = {4, 0.2f, 0.8f, 0.05f};
    int light_mode = RT_LIGHTS_UNIFORM;
    int grid_cells = 0, grid_clusters = 0;
    int indirect = 0;
    float orbit_d[2] = {0.0f, 0.0f};
    LightMove mv;
    rt_options opt;
    memset(&opt, 0, sizeof(opt));
    opt.max_depth = 6; opt.ris_sample_count = 32; opt.rejection_heuristics_threshold = 0.2f;
    opt.spatial_resampling_sample_count = 5; opt.spatial_resampling_radius = 30.0f;
    opt.spatial_resampling_passes = 3; opt.use_visibility_reuse = 1; /* common/options.hpp:6-22 */
    opt.use_temporal_resampling = 1; opt.use_spatial_resampling = 1;  /* keys 1, 2 */
    for (int i = 1; i < argc; ++i)
    {
        const std::string a = argv[i];
        auto f = [&](int k) { return (float)atof(argv[i + k]); };
        if (a == "--obj") obj = argv[++i];
        else if (a == "--tris") tris_path = argv[++i];
        else if (a == "--size") { W = atoi(argv[i + 1]); H = atoi(argv[i + 2]); i += 2; size_set = true; }
        else if (a == "--frames") frames = atoi(argv[++i]);
        else if (a == "--eye") { eye[0] = f(1); eye[1] = f(2); eye[2] = f(3); i += 3; cam_set = true; }
        else if (a == "--lookat") { lookat[0] = f(1); lookat[1] = f(2); lookat[2] = f(3); i += 3; cam_set = true; }
        else if (a == "--temporal") opt.use_temporal_resampling = (uint8_t)atoi(argv[++i]);
        else if (a == "--spatial") opt.use_spatial_resampling = (uint8_t)atoi(argv[++i]);
        else if (a == "--shadowed") opt.use_shadowed_target_function = (uint8_t)atoi(argv[++i]);
        else if (a == "--visreuse") opt.use_visibility_reuse = (uint8_t)atoi(argv[++i]);
        else if (a == "--accumulate") opt.accumulate = (uint8_t)atoi(argv[++i]);
        else if (a == "--by-kernel") by_kernel = true;
        else if (a == "--example") example = atoi(argv[++i]);
        else if (a == "--ranks") ranks = atoi(argv[++i]);
        else if (a == "--mirror") mirror = true;
        else if (a == "--shm") shm = true;
        else if (a == "--equal-strips") equal_strips = true;
        else if (a == "--cost-strips") equal_strips = false;
        else if (a == "--bounds")
        {
            std::stringstream ss(argv[++i]);
            std::string tok;
            while (std::getline(ss, tok, ',')) given_bounds.push_back(atoi(tok.c_str()));
        }
        else if (a == "--dump-tris") dump = argv[++i]; /* write the loaded triangle array and exit (no GPU needed) */
        else if (a == "--ppm") ppm = argv[++i];
        else if (a == "--png") png = argv[++i];
        else if (a == "--pfm") pfm = argv[++i];
        else if (a == "--rgba") rgba = argv[++i];
        else if (a == "--threads") threads = atoi(argv[++i]);
        else if (a == "--denoise") denoise = atoi(argv[++i]);
        else if (a == "--denoise-temporal") denoise_temporal = true;
        else if (a == "--unbiased") unbiased = true;
        else if (a == "--reproject") reproject = true;
        else if (a == "--unbiased-temporal") unbiased_temporal = true;
        else if (a == "--follow-motion") follow_motion = true;
        else if (a == "--follow-lights") follow_lights = true;
        else if (a == "--denoise-follow-motion") denoise_follow = true;
        else if (a == "--denoise-antilag")
        {
            denoise_antilag = true;
            /* the four numbers are optional: taken if the next argument starts a number */
            if (i + 1 < argc && (isdigit((unsigned char)argv[i + 1][0]) || argv[i + 1][0] == '.'))
            {
                if (i + 4 >= argc) { fprintf(stderr, "--denoise-antilag takes no numbers or four: radius lo hi floor\n"); return 2; }
                antilag.radius = atoi(argv[i + 1]);
                antilag.gradient_lo = (float)atof(argv[i + 2]);
                antilag.gradient_hi = (float)atof(argv[i + 3]);
                antilag.floor = (float)atof(argv[i + 4]);
                antilag_given = true;
                i += 4;
            }
        }
        else if (a == "--indirect")
        {
            if (i + 1 >= argc) { fprintf(stderr, "--indirect N\n"); return 2; }
            indirect = atoi(argv[++i]);
            if (indirect < 1 || indirect > 32) { fprintf(stderr, "--indirect: 1..32 bounces\n"); return 2; }
        }
        else if (a == "--light-grid")
        {
            if (i + 2 >= argc) { fprintf(stderr, "--light-grid CELLS CLUSTERS\n"); return 2; }
            grid_cells = atoi(argv[++i]);
            grid_clusters = atoi(argv[++i]);
            if (grid_cells < 1 || grid_cells > 32 || grid_clusters < 1 || grid_clusters > 256) { fprintf(stderr, "--light-grid: 1..32 cells per axis and 1..256 clusters\n"); return 2; }
        }
        else if (a == "--light-sampling")
        {
            const std::string m = i + 1 < argc ? argv[++i] : "";
            if (m == "uniform") light_mode = RT_LIGHTS_UNIFORM;
            else if (m == "power") light_mode = RT_LIGHTS_POWER;
            else { fprintf(stderr, "--light-sampling uniform|power\n"); return 2; }
        }
        else if (a == "--orbit") { orbit_d[0] = f(1); orbit_d[1] = f(2); i += 2; orbit = true; }
        else if (a == "--move-lights") { mv.d[0] = f(1); mv.d[1] = f(2); mv.d[2] = f(3); i += 3; mv.on = true; move_lights_given = true; }
        else if (a == "--move-tris" && i + 5 < argc)
        {
            mv.first = (uint32_t)strtoul(argv[i + 1], nullptr, 10); mv.count = (uint32_t)strtoul(argv[i + 2], nullptr, 10);
            mv.d[0] = f(3); mv.d[1] = f(4); mv.d[2] = f(5); i += 5; mv.on = true; mv.all = true;
        }
        else { fprintf(stderr, "unknown argument %s\n", a.c_str()); return 2; }
    }
    if (denoise >= 0 && (example == 4 || example == 6)) { fprintf(stderr, "--denoise applies to --example 10, 7, 8 and 9\n"); return 2; }
    if (denoise >= 0 && ranks > 1) { fprintf(stderr, "--denoise runs on one GPU (whole-frame contexts), not with --ranks\n"); return 2; }
    if (denoise > 8) { fprintf(stderr, "--denoise: 0..8 iterations\n"); return 2; }
    if (denoise_temporal && denoise < 0) { fprintf(stderr, "--denoise-temporal needs --denoise N\n"); return 2; }
    if (unbiased && (ranks > 1 || example != 10)) { fprintf(stderr, "--unbiased applies to one GPU and --example 10\n"); return 2; }
    if (reproject && (ranks > 1 || example != 10)) { fprintf(stderr, "--reproject applies to one GPU and --example 10\n"); return 2; }
    if (denoise_follow && !denoise_temporal) { fprintf(stderr, "--denoise-follow-motion needs --denoise N --denoise-temporal\n"); return 2; }
    if (denoise_antilag && !denoise_temporal) { fprintf(stderr, "--denoise-antilag needs --denoise N --denoise-temporal\n"); return 2; }
    if (follow_lights && example != 10) { fprintf(stderr, "--follow-lights needs --example 10\n"); return 2; }
    if (follow_lights && ranks > 1) { fprintf(stderr, "--follow-lights applies to one GPU: strip contexts are not re-based\n"); return 2; }
    if (follow_motion && !reproject) { fprintf(stderr, "--follow-motion needs --reproject\n"); return 2; }
    if (unbiased_temporal && !reproject) { fprintf(stderr, "--unbiased-temporal needs --reproject\n"); return 2; }
    if (unbiased_temporal && follow_motion) { fprintf(stderr, "--unbiased-temporal and --follow-motion exclude each other\n"); return 2; }
    if (mv.all && move_lights_given) { fprintf(stderr, "--move-tris and --move-lights exclude each other\n"); return 2; }
    if (indirect && (ranks > 1 || example != 10)) { fprintf(stderr, "--indirect applies to one GPU and --example 10\n"); return 2; }
    if (grid_cells && (ranks > 1 || example != 10)) { fprintf(stderr, "--light-grid applies to one GPU and --example 10\n"); return 2; }
    if (light_mode != RT_LIGHTS_UNIFORM && example != 10) { fprintf(stderr, "--light-sampling applies to --example 10\n"); return 2; }
    if (orbit && (ranks > 1 || example == 4 || example == 6)) { fprintf(stderr, "--orbit applies to one GPU and --example 10, 7, 8 and 9\n"); return 2; }
    std::vector<rt_triangle> triangles = !obj.empty() ? load_obj(obj) : load_tris(tris_path);
    if (triangles.empty()) { fprintf(stderr, "no triangles (use --obj or --tris)\n"); return 2; }
    if (!dump.empty())
    {
        FILE* f = fopen(dump.c_str(), "wb");
        fwrite(triangles.data(), sizeof(rt_triangle), triangles.size(), f);
        fclose(f);
        printf("triangles: %zu\n", triangles.size());
        return 0;
    }

    if (example == 4)
    {
        /* BASELINE config #1: 04_ao as a host loop (host_path.h); no context, no GPU */
        if (!size_set) { W = 256; H = 256; }
        if (!cam_set) { eye[0] = eye[1] = eye[2] = 8.0f; lookat[0] = lookat[1] = lookat[2] = 0.0f; } /* common/misc.hpp:217-218 */
        if (ranks > 1) { fprintf(stderr, "--example 4 is a host loop: --threads, not --ranks\n"); return 2; }
        rt_raygen rg;
        rt_host::raygen_lookat(&rg, eye, lookat, up, 3.14159265358979323846f / 4.0f, W, H); /* 04_ao.cpp:124-135 */
        std::vector<uint8_t> px((size_t)W * H * 4);
        const auto t0 = std::chrono::steady_clock::now();
        rt_host::ao04_image(triangles.data(), (uint32_t)triangles.size(), rg, W, H, threads, px.data());
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        const unsigned hw = std::thread::hardware_concurrency();
        size_t hit = 0;
        for (size_t i = 0; i < (size_t)W * H; ++i) hit += px[4 * i] != 32 || px[4 * i + 1] != 32;
        printf("triangles: %zu\n04_ao %dx%d: %.1f ms on %d host thread(s), %zu of %zu pixels hit\n", triangles.size(), W, H, ms,
               threads > 0 ? threads : (int)(hw ? hw : 1), hit, (size_t)W * H);
        return write_ao_image(px, W, H, rgba, ppm, png);
    }
    if (example == 6)
    {
        /* BASELINE config #1 on the GPU: 06_ao_hiprt (= 04_ao's kernelMain) through rt_path_trace; defaults of 06_ao_hiprt.cpp:79-80 */
        if (!cam_set) { eye[0] = eye[1] = eye[2] = 8.0f; lookat[0] = lookat[1] = lookat[2] = 0.0f; }
        if (ranks > 1) { fprintf(stderr, "--example 6 runs on one GPU\n"); return 2; }
        if (frames < 1) frames = 1;
        rt_ctx* ctx = nullptr;
        int rc = rt_create(0, W, H, 0, H, 0, &ctx);
        if (rc != RT_OK) die(ctx, "rt_create", rc);
        CK(rt_scene_set(ctx, triangles.data(), (uint32_t)triangles.size()));
        CK(rt_camera_lookat(ctx, eye, lookat, up, 3.14159265358979323846f / 4.0f));
        CK(rt_path_trace(ctx, 6, 0)); /* warm-up */
        CK(rt_sync(ctx));
        const auto t0 = std::chrono::steady_clock::now();
        for (int k = 0; k < frames; ++k) CK(rt_path_trace(ctx, 6, 0));
        CK(rt_sync(ctx));
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / frames;
        uint64_t rays = 0;
        CK(rt_path_trace_rays(ctx, &rays));
        std::vector<uint8_t> px((size_t)W * H * 4);
        CK(rt_download(ctx, RT_BUF_PIXELS, px.data(), px.size()));
        CK(rt_destroy(ctx));
        printf("triangles: %zu\n06_ao_hiprt %dx%d: %.3f ms per launch (%d launches after one warm-up), %llu rays per launch, %.0f Mray/s\n",
               triangles.size(), W, H, ms, frames, (unsigned long long)rays, (double)rays / ms / 1e3);
        return write_ao_image(px, W, H, rgba, ppm, png);
    }
    if (example != 10 && example != 7 && example != 8 && example != 9) { fprintf(stderr, "--example 10, 7, 8, 9, 6 or 4\n"); return 2; }
    if (mv.on && example != 10) { fprintf(stderr, "--move-lights and --move-tris apply to --example 10\n"); return 2; }
    if (mv.all && (uint64_t)mv.first + mv.count > triangles.size()) { fprintf(stderr, "--move-tris: [%u, %llu) outside the scene's %zu triangles\n", mv.first, (unsigned long long)mv.first + mv.count, triangles.size()); return 2; }
    if (mv.on && !mv.all) light_span(triangles, mv);

    if (ranks > 1)
    {
        /* one process per GPU, forked BEFORE any HIP call (a process that has initialised the GPU must not fork) */
        if (ranks > 64 || example != 10) { fprintf(stderr, "--ranks: 2..64 ranks of the ReSTIR DI frame\n"); return 2; }
        const size_t bytes = sizeof(Shared) + (size_t)H * 4;
        Shared* sh = (Shared*)mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_SHARED | MAP_ANONYMOUS, -1, 0);
        if (sh == MAP_FAILED) { perror("mmap"); return 1; }
        memset((void*)sh, 0, bytes);
        if (!pfm.empty())
        {
            FILE* f = fopen(pfm.c_str(), "wb");
            if (!f) { fprintf(stderr, "cannot write %s\n", pfm.c_str()); return 1; }
            const int hl = fprintf(f, "PF\n%d %d\n-1.0\n", W, H);
            fclose(f);
            if (truncate(pfm.c_str(), (off_t)hl + (off_t)W * H * 12) != 0) { perror("truncate"); return 1; }
        }
        std::vector<pid_t> kids;
        for (int r = 0; r < ranks; ++r)
        {
            const pid_t pid = fork();
            if (pid == 0)
            {
                const int code = rank_main(r, ranks, mirror, shm, equal_strips, given_bounds, sh, triangles, W, H, frames, eye, lookat, opt, light_mode, pfm, mv);
                fflush(stdout);
                fflush(stderr);
                _exit(code); /* no atexit handlers of the parent's image in a forked child */
            }
            kids.push_back(pid);
        }
        int worst = 0;
        for (pid_t k : kids)
        {
            int status = 0;
            waitpid(k, &status, 0);
            const int code = WIFEXITED(status) ? WEXITSTATUS(status) : 1;
            worst = code > worst ? code : worst;
        }
        return worst;
    }

    rt_ctx* ctx = nullptr;
    int rc = rt_create(0, W, H, 0, H, 0, &ctx);
    if (rc != RT_OK) die(ctx, "rt_create", rc);
    CK(rt_scene_set(ctx, triangles.data(), (uint32_t)triangles.size()));
    uint32_t nt, nl, bh;
    CK(rt_scene_info(ctx, &nt, &nl, &bh));
    printf("triangles: %u\nlights: %u\nbvh height: %u\n", nt, nl, bh); /* cf. 10_restir_di.cpp:206 */
    CK(rt_camera_lookat(ctx, eye, lookat, up, 3.14159265358979323846f / 4.0f)); /* :242-251 */
    CK(rt_options_set(ctx, &opt));
    if (unbiased) CK(rt_spatial_unbiased(ctx, 1));
    if (reproject) CK(rt_temporal_reprojection(ctx, 1));
    if (follow_motion) CK(rt_temporal_motion(ctx, 1));
    if (follow_lights) CK(rt_temporal_light_motion(ctx, 1));
    if (unbiased_temporal) CK(rt_temporal_unbiased(ctx, 1));
    if (denoise_follow) CK(rt_denoise_temporal_motion(ctx, 1));
    if (denoise_antilag) CK(rt_denoise_temporal_antilag(ctx, 1, antilag_given ? &antilag : nullptr));
    CK(rt_light_sampling(ctx, light_mode));
    if (grid_cells) CK(rt_light_grid(ctx, grid_cells, grid_clusters));
    if (indirect) CK(rt_indirect(ctx, indirect));
    CK(rt_timing_enable(ctx, 1));
    CK(rt_clear(ctx)); /* :222-226 */

    for (int frame = 1; frame <= frames; ++frame) /* frame++ before the first launch, :233-234 */
    {
        int clear = 0;
        if (mv.on && frame >= 2 && mv.count > 0)
        {
            const double ms = move_lights(ctx, triangles, mv);
            printf("frame %d scene update: %.3f ms (%u triangles)\n", frame, ms, mv.count);
            if (frame == frames) print_bvh_cost(ctx);
            clear = opt.accumulate ? 1 : 0;
        }
        if (orbit && frame >= 2)
        {
            int updated = 0;
            CK(rt_camera_orbit(ctx, orbit_d[0], orbit_d[1]));
            CK(rt_camera_updated(ctx, &updated));
            if (updated && opt.accumulate) clear = 1; /* 10_restir_di.cpp:257-267 */
        }
        if (example != 10)
        {
            /* examples/07_pt/07_pt.cpp:206-222: path_trace, then tone_mapping */
            if (clear) CK(rt_clear(ctx));
            CK(rt_path_trace(ctx, example, frame));
            CK(rt_tone_mapping(ctx));
        }
        else if (!by_kernel) { CK(rt_frame(ctx, frame, clear, nullptr)); }
        else
        {
            if (clear) CK(rt_clear(ctx));
            /* the launch sequence of 10_restir_di.cpp:270-379, one C-ABI call per kernel */
            CK(rt_raycast(ctx));
            CK(rt_generate_candidate(ctx, frame, RT_RES_0));
            CK(rt_temporal_resampling(ctx, frame, RT_RES_TEMPORAL, RT_RES_0));
            CK(rt_save_temporal_reservoir(ctx, RT_RES_0, RT_RES_TEMPORAL));
            int in = RT_RES_0, out = RT_RES_1;
            for (int k = 0; k < opt.spatial_resampling_passes; ++k)
            {
                if (k != 0) { const int t = in; in = out; out = t; }
                CK(rt_spatial_resampling(ctx, frame, k, in, out));
            }
            CK(rt_resolve(ctx, out));
            if (indirect) CK(rt_indirect_pass(ctx, frame, indirect));
            CK(rt_tone_mapping(ctx));
        }
        if (denoise >= 0)
        {
            rt_denoise_params dp = {denoise, 4.0f, 1.0f, 7, 3};
            if (denoise_temporal) CK(rt_denoise_temporal(ctx, &dp, nullptr));
            else CK(rt_denoise(ctx, &dp));
        }
        CK(rt_sync(ctx));
        if (!by_kernel && example == 10)
        {
            float ms[9];
            CK(rt_timing(ctx, ms));
            printf("frame %d kernel: %.3f ms (raycast %.3f, candidates %.3f, spatial %.3f+%.3f+%.3f, resolve %.3f)\n", frame,
                   ms[8], ms[1], ms[2], ms[3], ms[4], ms[5], ms[6]); /* cf. the overlay of :410 */
        }
        if (denoise_temporal)
        {
            float tms[6];
            CK(rt_denoise_temporal_timing(ctx, tms));
            printf("frame %d denoise: %.3f ms (guide %.3f, reprojection %.3f, variance %.3f, %d iterations %.3f)", frame, tms[5], tms[0], tms[1],
                   tms[2], denoise, tms[3] + tms[4]);
            if (denoise_follow)
            {
                int followed = 0;
                CK(rt_denoise_temporal_motion_get(ctx, nullptr, &followed));
                printf(followed ? " followed moved geometry" : " camera only");
            }
            if (denoise_antilag)
            {
                int adapted = 0;
                float al_ms = 0.0f;
                CK(rt_denoise_temporal_antilag_get(ctx, nullptr, nullptr, &adapted));
                if (adapted) CK(rt_denoise_temporal_antilag_timing(ctx, &al_ms));
                if (adapted) printf(" anti-lag adapted (%.3f ms)", al_ms);
                else printf(" anti-lag not adapted (no history)");
            }
            printf("\n");
        }
        else if (denoise >= 0)
        {
            float dms[5];
            CK(rt_denoise_timing(ctx, dms));
            printf("frame %d denoise: %.3f ms (guide %.3f, prep %.3f, %d iterations %.3f)\n", frame, dms[4], dms[0], dms[1], denoise, dms[2] + dms[3]);
        }
    }
    uint64_t rays = 0, shaded = 0;
    if (example == 10)
    {
        CK(rt_ray_count(ctx, &rays, &shaded));
        printf("rays/frame: %llu (shaded pixels %llu)\n", (unsigned long long)rays, (unsigned long long)shaded);
        if (follow_lights)
        {
            uint64_t lf[5] = {0, 0, 0, 0, 0};
            CK(rt_temporal_light_motion_stats(ctx, lf));
            printf("follow-lights: %llu buffers re-based; records examined %llu, located %llu, moved %llu, emptied %llu\n", (unsigned long long)lf[0],
                   (unsigned long long)lf[1], (unsigned long long)lf[2], (unsigned long long)lf[3], (unsigned long long)lf[4]);
        }
    }
    else
    {
        CK(rt_path_trace_rays(ctx, &rays));
        printf("rays in the last frame: %llu\n", (unsigned long long)rays);
    }

    if (!rgba.empty())
    {
        std::vector<uint8_t> px((size_t)W * H * 4);
        CK(rt_download(ctx, RT_BUF_PIXELS, px.data(), px.size()));
        FILE* f = fopen(rgba.c_str(), "wb");
        if (!f) { fprintf(stderr, "cannot write %s\n", rgba.c_str()); return 1; }
        fwrite(px.data(), 1, px.size(), f);
        fclose(f);
    }
    if (!ppm.empty())
    {
        std::vector<uint8_t> px((size_t)W * H * 4);
        CK(rt_download(ctx, RT_BUF_PIXELS, px.data(), px.size()));
        FILE* f = fopen(ppm.c_str(), "wb");
        fprintf(f, "P6\n%d %d\n255\n", W, H);
        for (int y = H - 1; y >= 0; --y) /* storage is bottom-up (pixel_idx = x + (H-yi-1)*W) */
            for (int x = 0; x < W; ++x) fwrite(&px[4 * ((size_t)y * W + x)], 1, 3, f);
        fclose(f);
    }
    if (!png.empty())
    {
        std::vector<uint8_t> px((size_t)W * H * 4), rgb((size_t)W * H * 3);
        CK(rt_download(ctx, RT_BUF_PIXELS, px.data(), px.size()));
        for (int y = 0; y < H; ++y) /* storage is bottom-up */
            for (int x = 0; x < W; ++x)
                memcpy(&rgb[3 * ((size_t)y * W + x)], &px[4 * ((size_t)(H - 1 - y) * W + x)], 3);
        write_png(png.c_str(), W, H, rgb.data());
    }
    if (!pfm.empty())
    {
        std::vector<float> acc((size_t)W * H * 4);
        CK(rt_download(ctx, denoise >= 0 ? (int)RT_BUF_DENOISED : (int)RT_BUF_ACCUMULATION, acc.data(), acc.size() * 4));
        FILE* f = fopen(pfm.c_str(), "wb");
        fprintf(f, "PF\n%d %d\n-1.0\n", W, H);
        for (size_t i = 0; i < (size_t)W * H; ++i)
        {
            const float w = acc[4 * i + 3];
            const float rgb[3] = {acc[4 * i] / w, acc[4 * i + 1] / w, acc[4 * i + 2] / w};
            fwrite(rgb, 4, 3, f);
        }
        fclose(f);
    }
    CK(rt_destroy(ctx));
    return 0;
}
