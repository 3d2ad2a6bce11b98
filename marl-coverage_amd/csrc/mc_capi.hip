// mc_capi.hip — the extern "C" boundary of libmarlcov.so (include/marlcov.h).
// Owns the device state of a batch of envs and launches mc_kernels.hip.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "marlcov.h"
#include "mc_internal.h"
#include "mc_beams.h"
#include "mc_config.h"
#include "mc_env_select.h"
#include "mc_export.h"
#include "mc_fork.h"
#include "mc_frontier.h"
#include "mc_fuse.h"
#include "mc_host.h"
#include "mc_import.h"
#include "mc_vistab.h"

namespace mc {
hipError_t launch_env(const State& s, int mode, const uint8_t* actions, const uint8_t* env_mask,
                      const int32_t* inj_pos, double* reward, uint8_t* done, uint8_t* obs,
                      uint8_t* adj, int num_steps, const EnvStrides& strides, int nt, int epw,
                      hipStream_t stream);
hipError_t launch_share(const State& s, const uint8_t* actions, hipStream_t stream);
hipError_t launch_rec_field(const State& s, int off, int width, void* buf, bool to_rec, hipStream_t stream);
hipError_t launch_pack(const State& s, const int8_t* grids, hipStream_t stream);
hipError_t launch_gen(const State& s, uint64_t seed, double p, hipStream_t stream);
hipError_t launch_random_actions(const State& s, uint64_t seed, int step, uint8_t* out, hipStream_t stream);
const char* env_variant(const State& s, int nt, int epw);
const char* env_label(const State& s, int nt, int epw);
bool env_takes_vis_table(const State& s, int nt, int epw);
hipError_t launch_dijkstra(const State& s, int pad, int layer, int Lc, uint8_t* obs,
                           uint32_t* list, bool window, uint64_t* big, unsigned big_slots,
                           hipStream_t stream);
hipError_t launch_dist(const State& s, int pad, int post, float* pre_out, float* dist_obs,
                       hipStream_t stream);
hipError_t launch_dist_listed(const State& s, int pad, float* pre_out, float* dist_obs,
                              uint32_t* list, uint32_t* count, uint32_t* full, hipStream_t stream);
hipError_t launch_frontier(const State& s, int pad, uint8_t* act, int32_t* dist, int32_t* goal,
                           uint32_t* list, bool window, uint64_t* big, unsigned big_slots,
                           hipStream_t stream);
hipError_t frontier_allow_lds(size_t lds);
size_t dist_lds_bytes(const State& s, int pad);
size_t dist_static_lds_bytes();
int dist_max_rows();
int dist_cache_max_rows();
size_t dijkstra_lds_bytes(const State& s, int pad);
size_t dijkstra_big_slot_bytes(const State& s, int pad);
unsigned dijkstra_big_slots(const State& s, int pad);
hipError_t launch_minimap(const State& s, int mini, double* out, hipStream_t stream);
hipError_t launch_export(const State& s, uint32_t layers, int scale, const int32_t* dev_envs, int count,
                         uint8_t* dev_out, hipStream_t stream);
hipError_t launch_import(const State& s, uint32_t layers, const int32_t* dev_envs, int count, const uint8_t* dev_in,
                         hipStream_t stream);
__global__ void dijkstra_kernel(State s, int pad, int layer, int Lc, uint8_t* obs_out,
                                const uint32_t* list, uint32_t* count);
}  // namespace mc

namespace {

using mc::fail;

struct Env {
  mc_config cfg;
  double range = 0.0;
  mc_layout lay;
  mc::State s;
  int device = -1;  // (-1: none yet, mc_create before its hipSetDevice)
  int nt = 128;
  int epw = 1;  // envs per workgroup (2: two envs share one wave)
  // steps per env-kernel launch of a fused mc_step_many call (MARLCOV_FUSE_STEPS,
  // read at mc_create; 1: one launch per step), and the env-kernel launches
  // this handle has issued (mc_env_launches)
  int fuse_steps = mc::kFuseStepsDefault;
  int64_t env_launches = 0;
  size_t dj_lds = 0;  // dijkstra_input: LDS bytes of the BFS kernel
  uint32_t* dj_list = nullptr;  // dijkstra_input: count, done, last count + [B*N] items (full-map BFS)
  bool dj_window = true;        // dijkstra_input: window kernel first (MARLCOV_DJ_FULL=1: off)
  uint64_t* dj_big = nullptr;   // dijkstra_input: the HBM kernel's plane scratch (null: the LDS kernel)
  unsigned dj_big_slots = 0;    // ... its slots = the HBM kernel's workgroups
  // mc_frontier_setup: the frontier call's own count words and item list (dj_list's
  // layout), its kernel choice, and the HBM kernel's scratch (a dijkstra_input
  // handle's own where it has one: the work is stream-ordered)
  bool fr_setup = false;
  uint32_t* fr_list = nullptr;
  bool fr_window = true;
  uint64_t* fr_big = nullptr;
  unsigned fr_big_slots = 0;
  size_t dt_lds = 0;  // dist_reward: LDS bytes of the distance kernel
  float* dist_pre = nullptr;  // dist_reward: [B][N][8] (library-owned)
  float* dist_obs = nullptr;  // dist_reward: caller's float32 [B][N][E][E]
  double* mini_obs = nullptr; // mini_map_rad: caller's float64 [B][N][2][E][E]
  uint32_t* dist_list = nullptr;  // dist_reward: (unused), workgroups done, last count, cache hits, last hits + the shards' maps (full transform)
  uint32_t* dist_full = nullptr;  // with the cache: the split transform's list (mc_dist.hip mode 2)
  bool dist_pre_stale = true;  // dist_pre does not describe the current maps
  bool beams_set = false;
  mc::DevBuf beams;    // mc::Beam [beam_count]
  mc::DevBuf bits;     // u64 [beam_count][max(Wp, Lp)]
  mc::DevBuf fan;      // u32 [State::fan_words]: fan march data (dense beam sets)
  mc::DevBuf rayprog;  // u32: the ray programs (State::ray_prog; common beam patterns)
  // the lidar's visibility table (State::vis_tab; mc_vistab.h): MARLCOV_VIS_TABLE
  // 0 off / 1 on (default) / 2 require, and MARLCOV_VIS_TABLE_MB, read at mc_create
  int vis_mode = 1;
  size_t vis_cap = 0;       // largest table to build, bytes
  mc::DevBuf vis;           // G x Wp x Lp records (allocated at the first build)
  int beam_count = 0;
  bool grids_set = false;
  std::vector<void*> allocs;
};

struct FieldDesc {
  void* ptr;
  int64_t bytes;
  int rec_off = -1;   // >= 0: a field of the env records (mc::EnvRec), not an array of its own
  int rec_width = 0;  // its bytes per env (4 or 8)
};

// copy a field between the env and the caller's contiguous buffer
int copy_field(Env* E, const FieldDesc& d, void* buf, bool to_env, hipStream_t st) {
  if (d.rec_off >= 0) {
    HIP_TRY(mc::launch_rec_field(E->s, d.rec_off, d.rec_width, buf, to_env, st));
    return MC_OK;
  }
  HIP_TRY(hipMemcpyAsync(to_env ? d.ptr : buf, to_env ? buf : d.ptr, (size_t)d.bytes, hipMemcpyDeviceToDevice, st));
  return MC_OK;
}

FieldDesc field(Env* E, int f) {
  const mc::State& s = E->s;
  const int64_t B = s.B, N = s.N, mw = s.MT, G = s.G;
#define REC_FIELD(name) \
  FieldDesc { s.rec, B * (int64_t)sizeof(s.rec->name), (int)offsetof(mc::EnvRec, name), (int)sizeof(s.rec->name) }
  switch (f) {
    case MC_FIELD_POS: return {s.pos, B * N * 2 * 4};
    case MC_FIELD_MOVED: return REC_FIELD(moved);
    case MC_FIELD_FREE: return {s.freem, B * N * mw * 8};
    case MC_FIELD_OBST: return {s.obstm, B * N * mw * 8};
    case MC_FIELD_VISITED: return {s.vis, B * mw * 8};
    case MC_FIELD_FREE_COUNT: return REC_FIELD(free_cnt);
    case MC_FIELD_VISITED_COUNT: return REC_FIELD(vis_cnt);
    case MC_FIELD_CURRSTEP: return REC_FIELD(currstep);
    case MC_FIELD_DONE_THRESH: return REC_FIELD(done_thresh);
    case MC_FIELD_ENV_GRID: return REC_FIELD(env_grid);
    case MC_FIELD_EPISODE: return REC_FIELD(episode);
    case MC_FIELD_NUMFREE: return {(void*)s.numfree, G * 4};
    case MC_FIELD_GRID_NEG: return {(void*)s.grid_neg, G * mw * 8};
    case MC_FIELD_GRID_POS: return {(void*)s.grid_pos, G * mw * 8};
    case MC_FIELD_DIST_MW: return {s.dist_mw, s.dist_mw ? B * N * 8 : -1};
    case MC_FIELD_DIST_LISTED: return {E->dist_list ? E->dist_list + 2 : nullptr, E->dist_list ? 4 : -1};
    case MC_FIELD_DIST_CACHED: return {E->dist_list ? E->dist_list + 4 : nullptr, E->dist_list ? 4 : -1};
    case MC_FIELD_EP_PC: return {s.ep_pc, B * 8};
    case MC_FIELD_EP_LEN: return {s.ep_len, B * 4};
    case MC_FIELD_DJ_LISTED: return {E->dj_list ? E->dj_list + 2 : nullptr, E->dj_list ? 4 : -1};
    case MC_FIELD_DIST_TOTALS: return {s.dist_tot, s.dist_tot ? 32 : -1};
    default: return {nullptr, -1};
  }
#undef REC_FIELD
}

Env* as_env(void* p) { return static_cast<Env*>(p); }

// envs per workgroup for this launch; MARLCOV_EPW=1 forces one env per
// workgroup (A/B tuning)
int launch_epw(const Env* E) {
  static const int force = [] {
    const char* v = getenv("MARLCOV_EPW");
    return v ? atoi(v) : 0;
  }();
  return force == 1 ? 1 : E->epw;
}

// (Re)build the visibility table on `st` after the pool or the beam table
// changed -- once both are there -- or drop it when this state's step kernel
// would not read one (no ray programs, another shape), the pool's table
// exceeds MARLCOV_VIS_TABLE_MB or its allocation fails: the step then marches,
// unless MARLCOV_VIS_TABLE=require asks for an error instead.
int vis_refresh(Env* E, hipStream_t st, const char* who) {
  mc::State& s = E->s;
  s.vis_tab = nullptr;
  if (E->vis_mode == 0 || !E->beams_set || !E->grids_set) return MC_OK;
  const uint64_t cells = (uint64_t)s.G * s.Wp * s.Lp;
  const uint64_t bytes = cells * mc::kVisRecWords * 4;
  char why[160] = "";
  if (s.sensor != MC_SENSOR_LIDAR || !mc::vis_fits(s.H) || !mc::env_takes_vis_table(s, E->nt, launch_epw(E)))
    snprintf(why, sizeof(why), "no step kernel of this shape and beam table reads a visibility table");
  else if (cells >= (1ull << 31) || bytes > E->vis_cap)
    snprintf(why, sizeof(why), "the pool's table of %llu MB exceeds MARLCOV_VIS_TABLE_MB = %llu",
             (unsigned long long)(bytes >> 20), (unsigned long long)(E->vis_cap >> 20));
  else if (!E->vis.p && E->vis.reserve((size_t)bytes) != hipSuccess) {
    (void)hipGetLastError();  // (cleared: the fallback is not an error)
    snprintf(why, sizeof(why), "allocating the table's %llu MB failed", (unsigned long long)(bytes >> 20));
  }
  if (why[0]) return E->vis_mode == 2 ? fail(MC_EINVAL, "%s: MARLCOV_VIS_TABLE=require, but %s", who, why) : MC_OK;
  HIP_TRY(mc::launch_vis_build(s, (uint32_t*)E->vis.p, st));
  s.vis_tab = (const uint32_t*)E->vis.p;
  return MC_OK;
}

// lanes per env workgroup and envs per workgroup for the current state
// (mc_create, and again when mc_set_beam_table changes the beam count)
void set_launch_shape(Env* E) {
  const char* ov = getenv("MARLCOV_NT");  // tuning / test override (64..1024)
  const mc::EnvGeom g = mc::env_geometry(E->s, ov ? atoi(ov) : 0);
  E->nt = g.nt;
  E->epw = g.epw;
}

// mc_create's switches, per handle (not cached: tests set them per env): the
// visibility table's and the fused launches'
void read_switches(Env* E) {
  if (const char* v = getenv("MARLCOV_VIS_TABLE")) E->vis_mode = v[0] == '0' ? 0 : (strcmp(v, "require") == 0 ? 2 : 1);
  E->vis_cap = (size_t)16384 << 20;
  if (const char* v = getenv("MARLCOV_VIS_TABLE_MB")) E->vis_cap = (size_t)strtoull(v, nullptr, 10) << 20;
  E->fuse_steps = mc::fuse_steps_from_env(getenv("MARLCOV_FUSE_STEPS"));
}

// The BFS kernel of dijkstra_input or the frontier call (`who`): the bitboards
// of one (env, agent) live in one workgroup's LDS where they fit (*lds: their
// bytes); else (or with MARLCOV_DJ_BIG=1: tests of the HBM kernel at small
// shapes) in an HBM scratch, a slot per workgroup of the HBM kernel (*lds = 0;
// allocated here unless `scratch` names one already)
int choose_bfs(Env* E, const char* who, size_t* lds, uint64_t*& scratch, unsigned& slots) {
  const mc::State& s = E->s;
  const mc_config& c = E->cfg;
  *lds = mc::dijkstra_lds_bytes(s, c.pad);
  int maxlds = 0;
  if (hipDeviceGetAttribute(&maxlds, hipDeviceAttributeMaxSharedMemoryPerBlock, E->device) != hipSuccess)
    return fail(MC_EHIP, "%s: cannot query the device's LDS per workgroup", who);
  if (*lds + 1024 <= (size_t)maxlds && !mc::env_is_1("MARLCOV_DJ_BIG")) return MC_OK;
  *lds = 0;
  if (scratch) return MC_OK;
  slots = mc::dijkstra_big_slots(s, c.pad);
  const size_t bytes = (size_t)slots * mc::dijkstra_big_slot_bytes(s, c.pad);
  if (mc::dev_alloc(E->allocs, scratch, bytes / 8) != MC_OK)
    return fail(MC_EHIP, "%s: %zu B of scratch (%u slots) for a %dx%d grid: %s", who, bytes, slots, c.width, c.length,
                mc::g_last_error.c_str());
  E->lay.state_bytes += (int64_t)bytes;
  return MC_OK;
}

const char* bfs_name(bool window, bool big) { return window ? (big ? "window+hbm" : "window+lds") : (big ? "hbm" : "lds"); }

// mc_create with dijkstra_input: the BFS kernel's choice, its scratch and its item list
int setup_dijkstra(Env* E) {
  const mc::State& s = E->s;
  const mc_config& c = E->cfg;
  // the end point of a path is the int32 cell index u * RY + v of the extended grid
  if (((int64_t)s.Wp + 2 * c.pad) * ((int64_t)s.Lp + 2 * c.pad) > INT32_MAX)
    return fail(MC_EINVAL, "dijkstra_input: the %dx%d grid's extended cells exceed a 32-bit index", c.width, c.length);
  if (int rc = choose_bfs(E, "dijkstra_input", &E->dj_lds, E->dj_big, E->dj_big_slots); rc != MC_OK) return rc;
  if (mc::dev_alloc(E->allocs, E->dj_list, (size_t)s.B * s.N + 3) != MC_OK)
    return fail(MC_EHIP, "dijkstra_input state: %s", mc::g_last_error.c_str());
  E->dj_window = !mc::env_is_1("MARLCOV_DJ_FULL");  // parity tests: every item on the full map
  if (!E->dj_window) {
    // no list, no count protocol: every step sends all B * N items to the full-map
    // kernel, and MC_FIELD_DJ_LISTED (count word 2, which no kernel then writes) says so
    const uint32_t all = (uint32_t)((size_t)s.B * s.N);
    HIP_TRY(hipMemcpy(E->dj_list + 2, &all, sizeof all, hipMemcpyHostToDevice));
  }
  return MC_OK;
}

// mc_create with dist_reward: the transform's limits, its terms and work
// lists, and the top-cell cache where it applies
int setup_dist(Env* E) {
  mc::State& s = E->s;
  const mc_config& c = E->cfg;
  if (c.width + c.length + 4 * c.pad >= 65535)
    return fail(MC_EINVAL, "dist_reward: grid %dx%d too large for 16-bit distances", c.width, c.length);
  if (s.Wp + 2 * c.pad > mc::dist_max_rows())
    return fail(MC_EINVAL, "dist_reward: %d extended rows exceed the transform's %d", s.Wp + 2 * c.pad,
                mc::dist_max_rows());
  if (s.Lp + 2 * c.pad > 32767)  // the witness column is a signed 16-bit half (mc_device.h)
    return fail(MC_EINVAL, "dist_reward: %d extended columns exceed 32767", s.Lp + 2 * c.pad);
  const size_t need = mc::dist_lds_bytes(s, c.pad);
  int maxlds = 0;
  if (hipDeviceGetAttribute(&maxlds, hipDeviceAttributeMaxSharedMemoryPerBlock, E->device) != hipSuccess ||
      need + mc::dist_static_lds_bytes() + 1024 > (size_t)maxlds)
    return fail(MC_EINVAL, "dist_reward: %zu B of LDS bitboards for a %dx%d grid exceed the "
                "device's %d B per workgroup", need, c.width, c.length, maxlds);
  E->dt_lds = need;
  std::vector<void*>& A = E->allocs;
  const size_t maps = (size_t)s.B * s.N;
  if (int rc = mc::dev_alloc(A, E->dist_pre, maps * 8); rc != MC_OK) return rc;
  s.dist_pre = E->dist_pre;
  // (M, witness) per map, M = -1 (unknown) until a full transform; the
  // work list of the full transform and its count
  const size_t cap = (size_t)((s.B + mc::kListShards - 1) / mc::kListShards) * s.N;  // entries per shard
  if (mc::dev_alloc(A, s.dist_mw, maps * 2, 0xFF) || mc::dev_alloc(A, E->dist_list, mc::kListShards * cap + 5) ||
      mc::dev_alloc(A, s.dist_tot, 4) || mc::dev_alloc(A, s.dist_shc, (size_t)mc::kListShards * mc::kShardStride))
    return fail(MC_EHIP, "dist_reward state: %s", mc::g_last_error.c_str());
  s.dist_cnt = E->dist_list;
  s.dist_cap = (uint32_t)cap;
  // the top-cell cache (mc_dist.hip), off with map sharing (other agents'
  // maps add cells outside the agent's own sensing windows) or
  // MARLCOV_DIST_CACHE=0, and off for maps past the LDS-bitboard transform's
  // rows (the big-map kernel transforms every listed map whole, mc_dist.hip)
  if (c.map_sharing || mc::env_starts_0("MARLCOV_DIST_CACHE") || s.Wp + 2 * c.pad > mc::dist_cache_max_rows())
    return MC_OK;
  const size_t gparts = (size_t)mc::kDistGSlots * mc::kDistGParts;
  uint32_t* full = nullptr;
  if (mc::dev_alloc(A, s.dist_cc, maps * mc::kDistK) || mc::dev_alloc(A, s.dist_cd, maps * mc::kDistK) ||
      mc::dev_alloc(A, s.dist_ch, maps * 8, 0xFF) || mc::dev_alloc(A, s.dist_sm, maps * mc::kDistStrips) ||
      mc::dev_alloc(A, s.dist_gkey, maps) || mc::dev_alloc(A, s.dist_gcnt, gparts) ||
      mc::dev_alloc(A, s.dist_pcnt, maps) || mc::dev_alloc(A, s.dist_govf, (size_t)mc::kDistGSlots) ||
      mc::dev_alloc(A, s.dist_rmask, maps) || mc::dev_alloc(A, s.dist_gcand, gparts * mc::kDistK) ||
      mc::dev_alloc(A, full, maps * 2 + 8))
    return fail(MC_EHIP, "dist_reward cache: %s", mc::g_last_error.c_str());
  // MARLCOV_DIST_SPLIT=0: every listed map's full transform in one workgroup
  if (!mc::env_starts_0("MARLCOV_DIST_SPLIT")) E->dist_full = s.dist_full = full;
  return MC_OK;
}

}  // namespace

extern "C" {

int32_t mc_abi_version(void) { return MARLCOV_ABI_VERSION; }

const char* mc_last_error(void) { return mc::g_last_error.c_str(); }

int64_t mc_struct_size(int32_t which) {
  switch (which) {
    case 0: return (int64_t)sizeof(mc_config);
    case 1: return (int64_t)sizeof(mc_layout);
    case 2: return (int64_t)sizeof(mc_sg_config);
    case 3: return (int64_t)sizeof(mc_sg_layout);
    default: return -1;
  }
}

int64_t mc_build_param(int32_t which) {
  switch (which) {
    case MC_PARAM_DIST_CACHE_CELLS: return mc::kDistK;
    case MC_PARAM_DIST_T: return mc::kDistT;
    case MC_PARAM_DIST_MAX_ROWS: return mc::dist_max_rows();
    default: return -1;
  }
}

int mc_create(const mc_config* cfg, int hip_device, void** out_env) {
  if (!cfg || !out_env) return fail(MC_EINVAL, "mc_create: null argument");
  *out_env = nullptr;
  const mc_config& c = *cfg;
  std::string err;
  if (!mc::check_config(c, err)) return fail(MC_EINVAL, "%s", err.c_str());
  std::unique_ptr<Env, mc::HandleDeleter<mc_destroy>> E(new Env());
  E->cfg = c;
  read_switches(E.get());
  const int H = mc::window_half(c);
  if (E->vis_mode == 2 && (c.sensor_type != MC_SENSOR_LIDAR || !mc::vis_fits(H)))
    return fail(MC_EINVAL, "mc_create: MARLCOV_VIS_TABLE=require, but a visibility record holds a lidar of "
                "half-width <= %d only (this env: %s, H = %d)", (mc::kVisRows - 1) / 2,
                c.sensor_type == MC_SENSOR_LIDAR ? "lidar" : "square sensor", H);
  E->range = c.lidar_range;
  mc::State& s = E->s;
  mc::derive_state(c, s);
  if (const hipError_t he = hipSetDevice(hip_device); he != hipSuccess)
    return fail(MC_EHIP, "hipSetDevice(%d): %s", hip_device, hipGetErrorString(he));
  E->device = hip_device;
  const size_t B = s.B, N = s.N, mw = (size_t)s.MT, G = s.G;
  size_t total = 0;
  int rc = MC_OK;
  auto alloc = [&](auto*& dst, size_t count) {
    total += count * sizeof(*dst);
    return rc = mc::dev_alloc(E->allocs, dst, count);
  };
  // one extra tile past each mask array stays zero: the env kernel's staged
  // tiles outside the map read it (no select on the loaded value)
  if (alloc(s.grid_neg, G * mw) || alloc(s.grid_pos, G * mw) || alloc(s.numfree, G) || alloc(s.rec, B) ||
      alloc(s.pos, B * N * 2) || alloc(s.freem, B * N * mw + 1) || alloc(s.obstm, B * N * mw + 1) ||
      alloc(s.vis, B * mw + 1) || alloc(s.err, 4) || alloc(s.ep_pc, B) || alloc(s.ep_len, B))
    return rc;
  std::vector<mc::EnvRec> recs(B);  // (value-initialised: zero)
  for (size_t i = 0; i < B; ++i) {
    recs[i].env_grid = (int32_t)(i % G);
    recs[i].done_thresh = c.done_thresh;
  }
  if (hipMemcpy(s.rec, recs.data(), B * sizeof(mc::EnvRec), hipMemcpyHostToDevice) != hipSuccess)
    return fail(MC_EHIP, "mc_create: initial upload failed");
  set_launch_shape(E.get());
  mc_layout& L = E->lay;
  L.tile_rows = 4 * s.TRS;
  L.tile_cols = 4 * s.TCS;
  L.window_half = s.H;
  L.window_tiles = s.TW;
  L.obs_layers = s.Lc;
  L.obs_side = s.E;
  L.obs_bytes_per_env = (int64_t)N * s.Lc * s.E * s.E;
  L.mask_words_per_agent = (int64_t)mw;
  // (the base arrays, and setup_dijkstra adds its HBM scratch; not the dist_reward arrays)
  L.state_bytes = (int64_t)total;
  if (c.dijkstra_input && (rc = setup_dijkstra(E.get())) != MC_OK) return rc;
  if (c.dist_reward && (rc = setup_dist(E.get())) != MC_OK) return rc;
  if (s.sensor != MC_SENSOR_LIDAR) E->beams_set = true;
  *out_env = E.release();
  return MC_OK;
}

void mc_destroy(void* env) {
  Env* E = as_env(env);
  if (!E) return;
  if (E->device >= 0) (void)hipSetDevice(E->device);
  for (void* p : E->allocs) (void)hipFree(p);
  delete E;  // (and its DevBufs)
}

int mc_query(void* env, mc_layout* out) {
  if (!env || !out) return fail(MC_EINVAL, "mc_query: null argument");
  *out = as_env(env)->lay;
  return MC_OK;
}

// u32 words into a buffer the handle grows as needed
static int upload_words(mc::DevBuf& buf, const std::vector<uint32_t>& w) {
  HIP_TRY(buf.reserve(w.size() * 4));
  HIP_TRY(hipMemcpy(buf.p, w.data(), w.size() * 4, hipMemcpyHostToDevice));
  return MC_OK;
}

int mc_set_beam_table(void* env, const double* host_table, int32_t num_beams) {
  Env* E = as_env(env);
  if (!E || !host_table) return fail(MC_EINVAL, "mc_set_beam_table: null argument");
  mc::State& s = E->s;
  if (s.sensor != MC_SENSOR_LIDAR) return fail(MC_EINVAL, "beam table on a non-lidar env");
  if (num_beams < 1) return fail(MC_EINVAL, "beam table needs >= 1 beam");
  // the per-env LDS budget mc_create checked holds 16 B per beam: a new beam
  // count must fit it too, or the next launch would fail inside HIP
  const int rb = s.TW <= 4 ? 4 : 8;
  if (mc::env_lds_bytes(s.N, s.TW, num_beams, rb) > 65536)
    return fail(MC_EINVAL, "mc_set_beam_table: %d beams exceed the 64 KiB per-env LDS window", num_beams);
  mc::BeamTables T;
  std::string err;
  if (!mc::compile_beams(host_table, num_beams, E->range, s.H, s.Wp, s.Lp, T, err))
    return fail(MC_EINVAL, "%s", err.c_str());
  HIP_TRY(hipSetDevice(E->device));
  // a queued launch (on any stream) may still read the tables: let it finish
  // before they are overwritten or freed.  Until the new tables are complete
  // the handle has none (a failure below leaves mc_step refusing to run
  // rather than reading freed or half-written tables).
  HIP_TRY(hipDeviceSynchronize());
  E->beams_set = false;
  s.fan_nsec = s.fan_nspec = s.fan_kt = s.fan_words = 0;
  s.fan_data = nullptr;
  s.ray_prog = nullptr;
  s.vis_tab = nullptr;
  const size_t bt_bytes = (size_t)num_beams * sizeof(mc::Beam), bits_bytes = T.bits.size() * sizeof(uint64_t);
  if (num_beams != E->beam_count || !E->beams.p) {
    // the reference lets callers swap _thetalist after construction
    // (even beam counts): (re-)size the device tables
    E->beam_count = 0;
    E->beams.release();
    E->bits.release();
    HIP_TRY(E->beams.reserve(bt_bytes));
    HIP_TRY(E->bits.reserve(bits_bytes));
    E->beam_count = num_beams;
    s.beams = (const mc::Beam*)E->beams.p;
    s.beam_bits = (const uint64_t*)E->bits.p;
    s.bcmax = T.cmax;
    s.nbeams = num_beams;
    s.mg_nb = mc::magic_div((uint32_t)num_beams);
    E->cfg.num_beams = num_beams;
    set_launch_shape(E);
  }
  HIP_TRY(hipMemcpy(E->beams.p, T.bt.data(), bt_bytes, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(E->bits.p, T.bits.data(), bits_bytes, hipMemcpyHostToDevice));
  // MARLCOV_BEAM_TABLE: march from the per-start tables, no fan; MARLCOV_NO_K1:
  // no step-1 premark; MARLCOV_FAN=0: the ray march (parity A/B), per call
  const bool per_start = getenv("MARLCOV_BEAM_TABLE") != nullptr, no_k1 = getenv("MARLCOV_NO_K1") != nullptr;
  const bool fan_off = per_start || mc::env_starts_0("MARLCOV_FAN");
  s.beam_kmax = T.kmax;
  s.beam_kmin = T.kmin;
  s.beam_common = T.common && !per_start ? 1 : 0;
  s.beam_k1 = s.beam_common && !no_k1 ? T.k1 : 0u;
  // ray programs of the launch geometry (set_launch_shape above, or
  // mc_create's: only a new beam count changes it), for common patterns
  std::vector<uint32_t> words;
  if (const int epw = s.beam_common ? launch_epw(E) : 0;
      epw && mc::build_ray_prog(T.bt, s.N, mc::ray_lpe(E->nt, epw), mc::ray_rpl(E->nt, epw, s.N, num_beams), T.kmax, rb,
                                words)) {
    if (int rc = upload_words(E->rayprog, words); rc != MC_OK) return rc;
    s.ray_prog = (const uint32_t*)E->rayprog.p;
  }
  // fan march of a dense set (after nt / epw: they bound the special lanes)
  int nsec = 0, nspec = 0;
  if (!fan_off && mc::build_fan(T, s.Wp, s.Lp, s.N, E->nt / E->epw, words, nsec, nspec) &&
      mc::env_lds_bytes(s.N, s.TW, num_beams, rb, mc::fan_lds_bytes(s.N, nspec, T.kmax, (int)words.size())) <= 65536) {
    if (int rc = upload_words(E->fan, words); rc != MC_OK) return rc;
    s.fan_data = (const uint32_t*)E->fan.p;
    s.fan_nsec = nsec;
    s.fan_nspec = nspec;
    s.fan_kt = T.kmax;
    s.fan_words = (int)words.size();
  }
  E->beams_set = true;
  // the visibility table of the new beams (the null stream; done before the
  // call returns, as the tables above are)
  if (int rc = vis_refresh(E, nullptr, "mc_set_beam_table"); rc != MC_OK) return rc;
  HIP_TRY(hipDeviceSynchronize());
  return MC_OK;
}

static int check_numfree(Env* E, hipStream_t st) {
  std::vector<int32_t> nf(E->s.G);
  HIP_TRY(hipMemcpyAsync(nf.data(), E->s.numfree, nf.size() * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  for (int g = 0; g < E->s.G; ++g)
    if (nf[g] <= 0)
      return fail(MC_EINVAL,
                  "grid %d has no cell > 0: the reference's percent_covered() divides by "
                  "count_nonzero(grid > 0) (dec_grid_rl.py:552)",
                  g);
  E->grids_set = true;
  return MC_OK;
}

int mc_set_grids(void* env, const int8_t* dev_grids, int32_t num_grids, void* stream) {
  Env* E = as_env(env);
  if (!E || !dev_grids) return fail(MC_EINVAL, "mc_set_grids: null argument");
  if (num_grids != E->s.G)
    return fail(MC_EINVAL, "mc_set_grids: %d grids, config says %d", num_grids, E->s.G);
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(E->device));
  HIP_TRY(hipMemsetAsync((void*)E->s.numfree, 0, (size_t)E->s.G * 4, st));
  HIP_TRY(mc::launch_pack(E->s, dev_grids, st));
  E->s.vis_tab = nullptr;  // the old pool's table is never read again
  if (int rc = check_numfree(E, st); rc != MC_OK) return rc;
  return vis_refresh(E, st, "mc_set_grids");
}

int mc_generate_grids(void* env, uint64_t seed, double p_obst, void* stream) {
  Env* E = as_env(env);
  if (!E) return fail(MC_EINVAL, "mc_generate_grids: null env");
  if (!(p_obst >= 0.0 && p_obst < 1.0)) return fail(MC_EINVAL, "p_obst must be in [0, 1)");
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(E->device));
  HIP_TRY(hipMemsetAsync((void*)E->s.numfree, 0, (size_t)E->s.G * 4, st));
  HIP_TRY(mc::launch_gen(E->s, seed, p_obst, st));
  E->s.vis_tab = nullptr;
  if (int rc = check_numfree(E, st); rc != MC_OK) return rc;
  return vis_refresh(E, st, "mc_generate_grids");
}

int mc_random_actions(void* env, uint64_t seed, int32_t step, uint8_t* dev_actions, void* stream) {
  Env* E = as_env(env);
  if (!E || !dev_actions) return fail(MC_EINVAL, "mc_random_actions: null argument");
  HIP_TRY(hipSetDevice(E->device));
  HIP_TRY(mc::launch_random_actions(E->s, seed, step, dev_actions, (hipStream_t)stream));
  return MC_OK;
}

const char* mc_kernel_variant(void* env) {
  Env* E = as_env(env);
  if (!E) return mc::fail_str(MC_EINVAL, "mc_kernel_variant: null env");
  // the lidar's march: "+fan(S/P)" = fan_march over S sectors and P special
  // beams (dense beam sets), else the ray march
  thread_local std::string name;
  name = mc::env_variant(E->s, E->nt, launch_epw(E));
  if (E->s.sensor == MC_SENSOR_LIDAR && E->s.fan_nsec + E->s.fan_nspec > 0)
    name += " +fan(" + std::to_string(E->s.fan_nsec) + "/" + std::to_string(E->s.fan_nspec) + ")";
  return name.c_str();
}

const char* mc_kernel_label(void* env) {
  Env* E = as_env(env);
  if (!E) return mc::fail_str(MC_EINVAL, "mc_kernel_label: null env");
  return mc::env_label(E->s, E->nt, launch_epw(E));
}

const char* mc_dijkstra_variant(void* env) {
  Env* E = as_env(env);
  if (!E) return mc::fail_str(MC_EINVAL, "mc_dijkstra_variant: null env");
  return E->cfg.dijkstra_input ? bfs_name(E->dj_window, E->dj_big) : "";
}

static_assert(mc::kFrontierEinval == MC_EINVAL && mc::kFrontierEstate == MC_ESTATE && mc::kActStay == MC_ACT_STAY,
              "mc_frontier.h restates marlcov.h's codes");

// The kernel choice of mc_create's dijkstra_input block, for the frontier call.
int mc_frontier_setup(void* env) {
  Env* E = as_env(env);
  const mc::FrontierCheck ck =
      mc::frontier_check_setup(E, E ? E->s.Wp : 0, E ? E->s.Lp : 0, E ? E->cfg.pad : 0);
  if (ck.rc) return fail(ck.rc, "%s", ck.msg);
  if (E->fr_setup) return MC_OK;
  const mc::State& s = E->s;
  HIP_TRY(hipSetDevice(E->device));
  // a dijkstra_input handle's scratch, sized by the same rule, serves both
  size_t need = 0;
  uint64_t* scratch = E->dj_big;
  unsigned slots = E->dj_big_slots;
  if (int rc = choose_bfs(E, "mc_frontier_setup", &need, scratch, slots); rc != MC_OK) return rc;
  if (need > 65536) HIP_TRY(mc::frontier_allow_lds(need));
  const size_t list_words = (size_t)s.B * s.N + 3;
  if (mc::dev_alloc(E->allocs, E->fr_list, list_words) != MC_OK)
    return fail(MC_EHIP, "mc_frontier_setup: item list: %s", mc::g_last_error.c_str());
  E->lay.state_bytes += (int64_t)list_words * 4;
  E->fr_big = need ? nullptr : scratch;
  E->fr_big_slots = need ? 0 : slots;
  E->fr_window = !mc::env_is_1("MARLCOV_DJ_FULL");
  HIP_TRY(hipDeviceSynchronize());  // the zeroed count words are there before any stream's first call
  E->fr_setup = true;
  return MC_OK;
}

const char* mc_frontier_variant(void* env) {
  Env* E = as_env(env);
  const mc::FrontierCheck ck = mc::frontier_check_variant(E);
  if (ck.rc) return mc::fail_str(ck.rc, ck.msg);
  return E->fr_setup ? bfs_name(E->fr_window, E->fr_big) : "";
}

int mc_frontier_actions(void* env, uint8_t* dev_actions, int32_t* dev_dist, int32_t* dev_goal, void* stream) {
  Env* E = as_env(env);
  const mc::FrontierCheck ck = mc::frontier_check_actions(E, dev_actions, E && E->fr_setup);
  if (ck.rc) return fail(ck.rc, "%s", ck.msg);
  HIP_TRY(hipSetDevice(E->device));
  HIP_TRY(mc::launch_frontier(E->s, E->cfg.pad, dev_actions, dev_dist, dev_goal, E->fr_list, E->fr_window,
                              E->fr_big, E->fr_big_slots, (hipStream_t)stream));
  return MC_OK;
}

int mc_set_env_grids(void* env, const int32_t* dev_env_grid, void* stream) {
  Env* E = as_env(env);
  if (!E || !dev_env_grid) return fail(MC_EINVAL, "mc_set_env_grids: null argument");
  HIP_TRY(hipSetDevice(E->device));
  HIP_TRY(mc::launch_rec_field(E->s, (int)offsetof(mc::EnvRec, env_grid), 4, const_cast<int32_t*>(dev_env_grid),
                               /*to_rec=*/true, (hipStream_t)stream));
  return MC_OK;
}

// dijkstra_input: obs layer 3 from the post-step maps (dec_grid_rl.py:354-358),
// a second kernel on the same stream
static int dijkstra_layer(Env* E, void* dev_obs, hipStream_t st) {
  if (E->cfg.mini_map_rad > 0) {  // the minimap overwrites layer 3 (dec_grid_rl.py:365)
    HIP_TRY(mc::launch_minimap(E->s, E->cfg.mini_map_rad, E->mini_obs, st));
    return MC_OK;
  }
  if (!E->cfg.dijkstra_input) return MC_OK;
  if (E->dj_lds > 65536)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&mc::dijkstra_kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)E->dj_lds));
  HIP_TRY(mc::launch_dijkstra(E->s, E->cfg.pad, 3, E->s.Lc, (uint8_t*)dev_obs, E->dj_list,
                              E->dj_window, E->dj_big, E->dj_big_slots, st));
  return MC_OK;
}

// dist_reward: the distance terms of the maps before sensing (PRE, read by
// the env kernel's reward) or the obs layer of the maps after it (POST)
static int dist_terms(Env* E, int post, hipStream_t st) {
  if (!E->cfg.dist_reward) return MC_OK;
  if (post)  // the full transform of the maps the env kernel listed (unknown max(d), or a
             // target its window search could not settle)
    HIP_TRY(mc::launch_dist_listed(E->s, E->cfg.pad, E->dist_pre, E->dist_obs, E->dist_list + 5,
                                   E->dist_list, E->dist_full, st));
  else
    HIP_TRY(mc::launch_dist(E->s, E->cfg.pad, 0, E->dist_pre, E->dist_obs, st));
  E->dist_pre_stale = !post;  // a POST transform leaves PRE data for the next step
  return MC_OK;
}

static int ready(Env* E, const char* who) {
  if (!E->beams_set) return fail(MC_ESTATE, "%s: lidar beam table not set (mc_set_beam_table)", who);
  if (!E->grids_set) return fail(MC_ESTATE, "%s: grids not set (mc_set_grids / mc_generate_grids)", who);
  if (E->cfg.dist_reward && !E->dist_obs)
    return fail(MC_ESTATE, "%s: dist_reward needs the float obs buffer (mc_set_dist_obs)", who);
  if (E->cfg.mini_map_rad > 0 && !E->mini_obs)
    return fail(MC_ESTATE, "%s: mini_map_rad needs the float64 minimap buffer (mc_set_minimap_obs)", who);
  return MC_OK;
}

int mc_reset(void* env, const uint8_t* dev_env_mask, const int32_t* dev_pos, void* dev_obs,
             uint8_t* dev_adj, void* stream) {
  Env* E = as_env(env);
  if (!E || !dev_obs) return fail(MC_EINVAL, "mc_reset: null argument");
  int rc = ready(E, "mc_reset");
  if (rc) return rc;
  HIP_TRY(hipSetDevice(E->device));
  HIP_TRY(mc::launch_env(E->s, mc::MODE_RESET, nullptr, dev_env_mask, dev_pos, nullptr, nullptr,
                         (uint8_t*)dev_obs, dev_adj, 1, mc::EnvStrides{}, E->nt, launch_epw(E), (hipStream_t)stream));
  ++E->env_launches;
  rc = dijkstra_layer(E, dev_obs, (hipStream_t)stream);
  if (rc) return rc;
  return dist_terms(E, 1, (hipStream_t)stream);
}

// the launches of one step (the caller checked the arguments and set the device)
static int step_once(Env* E, const uint8_t* dev_actions, double* dev_reward, uint8_t* dev_done,
                     void* dev_obs, uint8_t* dev_adj, hipStream_t st) {
  int rc;
  if (E->cfg.map_sharing) HIP_TRY(mc::launch_share(E->s, dev_actions, st));
  if (E->cfg.map_sharing || E->dist_pre_stale) {
    rc = dist_terms(E, 0, st);  // observe() reads the maps before sensing
    if (rc) return rc;
  }
  HIP_TRY(mc::launch_env(E->s, mc::MODE_STEP, dev_actions, nullptr, nullptr, dev_reward, dev_done,
                         (uint8_t*)dev_obs, dev_adj, 1, mc::EnvStrides{}, E->nt, launch_epw(E), st));
  ++E->env_launches;
  rc = dijkstra_layer(E, dev_obs, st);
  if (rc) return rc;
  return dist_terms(E, 1, st);
}

// mc_step_many runs several steps per env-kernel launch: the handle's step is
// the env kernel alone (no launch before or after it reads or writes the maps)
static bool fuses_steps(const Env* E) {
#ifdef MC_STAMPS
  return false;  // the phase stamps are per launch
#else
  return E->fuse_steps > 1 && !E->cfg.map_sharing && !E->cfg.dist_reward && !E->cfg.dijkstra_input &&
         E->cfg.mini_map_rad == 0;
#endif
}

int mc_step(void* env, const uint8_t* dev_actions, double* dev_reward, uint8_t* dev_done,
            void* dev_obs, uint8_t* dev_adj, void* stream) {
  Env* E = as_env(env);
  if (!E || !dev_actions || !dev_reward || !dev_done || !dev_obs)
    return fail(MC_EINVAL, "mc_step: null argument");
  int rc = ready(E, "mc_step");
  if (rc) return rc;
  HIP_TRY(hipSetDevice(E->device));
  return step_once(E, dev_actions, dev_reward, dev_done, dev_obs, dev_adj, (hipStream_t)stream);
}

int mc_step_many(void* env, const uint8_t* dev_actions, int64_t actions_stride, int32_t num_steps,
                 double* dev_reward, int64_t reward_stride, uint8_t* dev_done, int64_t done_stride,
                 void* dev_obs, int64_t obs_stride, uint8_t* dev_adj, int64_t adj_stride, void* stream) {
  Env* E = as_env(env);
  if (!E || !dev_actions || !dev_reward || !dev_done || !dev_obs)
    return fail(MC_EINVAL, "mc_step_many: null argument");
  if (num_steps < 0 || actions_stride < 0 || reward_stride < 0 || done_stride < 0 || obs_stride < 0 ||
      adj_stride < 0)
    return fail(MC_EINVAL, "mc_step_many: negative step count or stride");
  if (reward_stride % 8 != 0) return fail(MC_EINVAL, "mc_step_many: reward_stride must be a multiple of 8 bytes");
  int rc = ready(E, "mc_step_many");
  if (rc) return rc;
  HIP_TRY(hipSetDevice(E->device));
  hipStream_t st = (hipStream_t)stream;
  const int64_t stride[mc::FUSE_BUFS] = {actions_stride, reward_stride, done_stride, obs_stride, adj_stride};
  if (!mc::fuse_offsets_fit(num_steps, stride))
    return fail(MC_EINVAL, "mc_step_many: a stride times the step count overflows int64");
  if (fuses_steps(E)) {
    // the step is the env kernel alone: up to fuse_steps steps per launch
    const mc::EnvStrides es{actions_stride, reward_stride, done_stride, obs_stride, adj_stride};
    const int64_t chunks = mc::fuse_chunk_count(num_steps, E->fuse_steps);
    for (int64_t i = 0; i < chunks; ++i) {
      mc::FuseChunk c;
      if (!mc::fuse_chunk(num_steps, E->fuse_steps, i, stride, &c))
        return fail(MC_EINVAL, "mc_step_many: chunk %lld of %lld", (long long)i, (long long)chunks);
      const hipError_t he = mc::launch_env(
          E->s, mc::MODE_STEP, dev_actions + c.off[mc::FUSE_ACTIONS], nullptr, nullptr,
          reinterpret_cast<double*>(reinterpret_cast<char*>(dev_reward) + c.off[mc::FUSE_REWARD]),
          dev_done + c.off[mc::FUSE_DONE], static_cast<uint8_t*>(dev_obs) + c.off[mc::FUSE_OBS],
          dev_adj ? dev_adj + c.off[mc::FUSE_ADJ] : nullptr, c.count, es, E->nt, launch_epw(E), st);
      if (he != hipSuccess)  // the launches before it are enqueued: the env has advanced c.first steps
        return fail(MC_EHIP, "mc_step_many: step %lld of %d failed after %lld steps were enqueued: launch of %d steps: %s",
                    (long long)c.first, (int)num_steps, (long long)c.first, (int)c.count, hipGetErrorString(he));
      ++E->env_launches;
    }
    return MC_OK;
  }
  for (int32_t k = 0; k < num_steps; ++k) {
    rc = step_once(E, dev_actions + k * actions_stride,
                   reinterpret_cast<double*>(reinterpret_cast<char*>(dev_reward) + k * reward_stride),
                   dev_done + k * done_stride, static_cast<char*>(dev_obs) + k * obs_stride,
                   dev_adj ? dev_adj + k * adj_stride : nullptr, st);
    if (rc)  // steps 0..k-1 are enqueued: the env has advanced k steps
      return fail(rc, "mc_step_many: step %d of %d failed after %d steps were enqueued: %s", (int)k,
                  (int)num_steps, (int)k, mc::g_last_error.c_str());
  }
  return MC_OK;
}

int64_t mc_env_launches(void* env) {
  Env* E = as_env(env);
  if (!E) return fail(MC_EINVAL, "mc_env_launches: null env");
  return E->env_launches;
}

int64_t mc_field_bytes(void* env, int32_t f) {
  Env* E = as_env(env);
  if (!E) return fail(MC_EINVAL, "mc_field_bytes: null env");
  FieldDesc d = field(E, f);
  if (!d.ptr) return fail(MC_EINVAL, "unknown state field %d", f);
  return d.bytes;
}

int mc_get_state(void* env, int32_t f, void* dev_dst, int64_t bytes, void* stream) {
  Env* E = as_env(env);
  if (!E || !dev_dst) return fail(MC_EINVAL, "mc_get_state: null argument");
  FieldDesc d = field(E, f);
  if (!d.ptr) return fail(MC_EINVAL, "unknown state field %d", f);
  if (bytes != d.bytes) return fail(MC_EINVAL, "field %d is %lld bytes, got %lld", f, (long long)d.bytes, (long long)bytes);
  HIP_TRY(hipSetDevice(E->device));
  return copy_field(E, d, dev_dst, /*to_env=*/false, (hipStream_t)stream);
}

int mc_set_state(void* env, int32_t f, const void* dev_src, int64_t bytes, void* stream) {
  Env* E = as_env(env);
  if (!E || !dev_src) return fail(MC_EINVAL, "mc_set_state: null argument");
  FieldDesc d = field(E, f);
  if (!d.ptr) return fail(MC_EINVAL, "unknown state field %d", f);
  if (f == MC_FIELD_DIST_MW || f == MC_FIELD_DIST_LISTED || f == MC_FIELD_EP_PC || f == MC_FIELD_EP_LEN ||
      f == MC_FIELD_DJ_LISTED || f == MC_FIELD_DIST_CACHED || f == MC_FIELD_DIST_TOTALS)
    return fail(MC_EINVAL, "field %d is derived state (read-only)", f);
  if (bytes != d.bytes) return fail(MC_EINVAL, "field %d is %lld bytes, got %lld", f, (long long)d.bytes, (long long)bytes);
  HIP_TRY(hipSetDevice(E->device));
  if (int rc = copy_field(E, d, const_cast<void*>(dev_src), /*to_env=*/true, (hipStream_t)stream); rc != MC_OK) return rc;
  if (f == MC_FIELD_GRID_NEG || f == MC_FIELD_GRID_POS || f == MC_FIELD_NUMFREE) E->grids_set = true;
  if (f == MC_FIELD_GRID_NEG)  // an uploaded pool (a sibling's copy): its own visibility table
    if (int rc = vis_refresh(E, (hipStream_t)stream, "mc_set_state"); rc != MC_OK) return rc;
  E->dist_pre_stale = true;  // uploaded maps / positions: recompute the PRE terms
  if (E->s.dist_mw)  // and max(d) of every map
    HIP_TRY(hipMemsetAsync(E->s.dist_mw, 0xFF, (size_t)E->s.B * E->s.N * 8, (hipStream_t)stream));
  if (E->s.dist_ch)  // and the top-cell caches
    HIP_TRY(hipMemsetAsync(E->s.dist_ch, 0xFF, (size_t)E->s.B * E->s.N * 32, (hipStream_t)stream));
  return MC_OK;
}

int mc_copy_envs(void* dst, void* src, const int32_t* dev_src, void* stream) {
  Env* D = as_env(dst);
  Env* S = as_env(src);
  if (!D || !S || !dev_src) return fail(MC_EINVAL, "mc_copy_envs: null argument");
  const mc::State& d = D->s;
  const mc::State& s = S->s;
  if (S != D) {
    if (S->device != D->device)
      return fail(MC_EINVAL, "mc_copy_envs: handles on HIP devices %d and %d", D->device, S->device);
#define MC_SAME(what, a, b) \
  if ((a) != (b)) return fail(MC_EINVAL, "mc_copy_envs: %s differs (%d vs %d)", what, (int)(a), (int)(b))
    MC_SAME("num_agents", d.N, s.N);
    MC_SAME("width", d.Wp, s.Wp);
    MC_SAME("length", d.Lp, s.Lp);
    MC_SAME("pad", d.pad, s.pad);
    MC_SAME("num_grids", d.G, s.G);
    MC_SAME("dist_reward", d.dist_mw != nullptr, s.dist_mw != nullptr);
    MC_SAME("top-cell cache", d.dist_cc != nullptr, s.dist_cc != nullptr);
#undef MC_SAME
  }
  // Every per-env array that holds state between two calls.  The step's work
  // lists (dist_cnt / dist_shc, dist_full, dist_gkey, dist_gcnt, dist_pcnt,
  // dist_rmask, dj_list, the HBM dijkstra scratch) are filled and consumed
  // inside one mc_step / mc_reset and carry nothing over.
  const size_t N = d.N, mw = (size_t)d.MT;
  mc::ForkTable t;
  t.add(s.freem, d.freem, N * mw * 8);
  t.add(s.obstm, d.obstm, N * mw * 8);
  t.add(s.vis, d.vis, mw * 8);
  t.add(s.dist_cc, d.dist_cc, N * mc::kDistK * 4);
  t.add(s.dist_cd, d.dist_cd, N * mc::kDistK * 4);
  t.add(s.dist_sm, d.dist_sm, N * mc::kDistStrips * 4);
  t.add(s.dist_ch, d.dist_ch, N * 32);
  t.add(S->dist_pre, D->dist_pre, N * 8 * sizeof(float));
  t.add(s.dist_mw, d.dist_mw, N * 8);
  t.add(s.rec, d.rec, sizeof(mc::EnvRec));
  t.add(s.pos, d.pos, N * 8);
  t.add(s.ep_pc, d.ep_pc, 8);
  t.add(s.ep_len, d.ep_len, 4);
  HIP_TRY(hipSetDevice(D->device));
  HIP_TRY(mc::launch_fork(t, dev_src, s.B, d.B, S == D, d.err, mc::ERR_FORK, (hipStream_t)stream));
  // a fork sends no map to a transform that its source would not send
  D->dist_pre_stale = D->dist_pre_stale || S->dist_pre_stale;
  return MC_OK;
}

// planes / output bytes of an export, -1 (with the message) on a bad argument
static int64_t export_shape(Env* E, const char* who, uint32_t layers, int32_t scale, int32_t count, int* planes) {
  if (layers == 0 || (layers & ~mc::kMapAll))
    return fail(MC_EINVAL, "%s: layers 0x%x selects no plane or has unknown bits (MC_MAP_ALL = 0x%x)", who, layers,
                mc::kMapAll);
  if (scale != 1 && scale != 8) return fail(MC_EINVAL, "%s: scale %d is not 1 or 8", who, (int)scale);
  if (count < 0) return fail(MC_EINVAL, "%s: count %d is negative", who, (int)count);
  const mc::State& s = E->s;
  const int P = mc::export_planes(layers, s.N);
  const int64_t plane = scale == 8 ? (int64_t)s.TR * s.TC : (int64_t)s.Wp * s.Lp;
  if (plane * P >= 0x7FFFFFFFll)
    return fail(MC_EINVAL, "%s: layers 0x%x at scale %d are %lld bytes per env (limit 2 GiB)", who, layers,
                (int)scale, (long long)(plane * P));
  if (planes) *planes = P;
  return plane * P * (int64_t)count;
}

int32_t mc_map_planes(void* env, uint32_t layers) {
  Env* E = as_env(env);
  if (!E) return fail(MC_EINVAL, "mc_map_planes: null env");
  int P = 0;
  if (export_shape(E, "mc_map_planes", layers, 1, 0, &P) < 0) return MC_EINVAL;
  return P;
}

int64_t mc_export_bytes(void* env, uint32_t layers, int32_t scale, int32_t count) {
  Env* E = as_env(env);
  if (!E) return fail(MC_EINVAL, "mc_export_bytes: null env");
  return export_shape(E, "mc_export_bytes", layers, scale, count, nullptr);
}

int mc_export_maps(void* env, uint32_t layers, int32_t scale, const int32_t* dev_envs, int32_t count,
                   uint8_t* dev_out, int64_t out_bytes, void* stream) {
  Env* E = as_env(env);
  if (!E) return fail(MC_EINVAL, "mc_export_maps: null env");
  if (!dev_out) return fail(MC_EINVAL, "mc_export_maps: null dev_out");
  const int64_t bytes = export_shape(E, "mc_export_maps", layers, scale, count, nullptr);
  if (bytes < 0) return MC_EINVAL;
  if (!dev_envs && count != E->s.B)
    return fail(MC_EINVAL, "mc_export_maps: count %d with dev_envs NULL (NULL means all %d envs in order)",
                (int)count, E->s.B);
  if (out_bytes != bytes)
    return fail(MC_EINVAL, "mc_export_maps: out_bytes %lld, the output is %lld bytes (mc_export_bytes)",
                (long long)out_bytes, (long long)bytes);
  if ((uintptr_t)dev_out & 15u) return fail(MC_EINVAL, "mc_export_maps: dev_out %p is not 16-byte aligned", (void*)dev_out);
  if (!E->grids_set) return fail(MC_ESTATE, "mc_export_maps: grids not set (mc_set_grids / mc_generate_grids)");
  if (count == 0) return MC_OK;
  HIP_TRY(hipSetDevice(E->device));
  HIP_TRY(mc::launch_export(E->s, layers, scale, dev_envs, count, dev_out, (hipStream_t)stream));
  return MC_OK;
}

// input bytes of an import, -1 (with the message) on a bad argument
static int64_t import_shape(Env* E, const char* who, uint32_t layers, int32_t count) {
  if (layers == 0) return fail(MC_EINVAL, "%s: layers 0x0 selects no plane (MC_MAP_IMPORTABLE = 0x%x)", who, mc::kMapImportable);
  if (const uint32_t other = layers & ~mc::kMapImportable) {
    static const char* const names[7] = {"MC_MAP_GRID_NEG", "MC_MAP_GRID_POS", "MC_MAP_VISITED", "MC_MAP_OBST_ANY",
                                         "MC_MAP_ROBOTS",   "MC_MAP_FREE",     "MC_MAP_OBST"};
    const uint32_t bit = other & (0u - other);  // the lowest one
    const int b = __builtin_ctz(bit);
    if (b >= 7) return fail(MC_EINVAL, "%s: layers 0x%x has the unknown bit %u", who, layers, bit);
    return fail(MC_EINVAL, "%s: layers 0x%x has bit %u (%s), which %s (MC_MAP_IMPORTABLE = 0x%x)", who, layers, bit,
                names[b], b < 2 ? "belongs to the grid pool" : "is derived from the agents' maps", mc::kMapImportable);
  }
  if (count < 0) return fail(MC_EINVAL, "%s: count %d is negative", who, (int)count);
  const mc::State& s = E->s;
  const int P = mc::export_planes(layers, s.N);
  const int64_t plane = (int64_t)s.Wp * s.Lp;
  if (plane * P >= 0x7FFFFFFFll)
    return fail(MC_EINVAL, "%s: layers 0x%x are %lld bytes per env (limit 2 GiB)", who, layers, (long long)(plane * P));
  return plane * P * (int64_t)count;
}

int64_t mc_import_bytes(void* env, uint32_t layers, int32_t count) {
  Env* E = as_env(env);
  if (!E) return fail(MC_EINVAL, "mc_import_bytes: null env");
  return import_shape(E, "mc_import_bytes", layers, count);
}

int mc_import_maps(void* env, uint32_t layers, const int32_t* dev_envs, int32_t count, const uint8_t* dev_in,
                   int64_t in_bytes, void* stream) {
  Env* E = as_env(env);
  if (!E) return fail(MC_EINVAL, "mc_import_maps: null env");
  if (!dev_in) return fail(MC_EINVAL, "mc_import_maps: null dev_in");
  const int64_t bytes = import_shape(E, "mc_import_maps", layers, count);
  if (bytes < 0) return MC_EINVAL;
  if (!dev_envs && count != E->s.B)
    return fail(MC_EINVAL, "mc_import_maps: count %d with dev_envs NULL (NULL means all %d envs in order)",
                (int)count, E->s.B);
  if (in_bytes != bytes)
    return fail(MC_EINVAL, "mc_import_maps: in_bytes %lld, the input is %lld bytes (mc_import_bytes)",
                (long long)in_bytes, (long long)bytes);
  if (!E->grids_set) return fail(MC_ESTATE, "mc_import_maps: grids not set (mc_set_grids / mc_generate_grids)");
  if (count == 0) return MC_OK;
  HIP_TRY(hipSetDevice(E->device));
  HIP_TRY(mc::launch_import(E->s, layers, dev_envs, count, dev_in, (hipStream_t)stream));
  E->dist_pre_stale = true;  // imported maps / positions: recompute the PRE terms
  return MC_OK;
}

int mc_set_dist_obs(void* env, float* dev_dist_obs) {
  Env* E = as_env(env);
  if (!E || !dev_dist_obs) return fail(MC_EINVAL, "mc_set_dist_obs: null argument");
  if (!E->cfg.dist_reward) return fail(MC_EINVAL, "mc_set_dist_obs: config has dist_reward = 0");
  E->dist_obs = dev_dist_obs;
  E->s.dist_obs_out = dev_dist_obs;
  return MC_OK;
}

int mc_set_minimap_obs(void* env, double* dev_minimap_obs) {
  Env* E = as_env(env);
  if (!E || !dev_minimap_obs) return fail(MC_EINVAL, "mc_set_minimap_obs: null argument");
  if (E->cfg.mini_map_rad <= 0) return fail(MC_EINVAL, "mc_set_minimap_obs: config has mini_map_rad = 0");
  E->mini_obs = dev_minimap_obs;
  return MC_OK;
}

// Diagnostic builds only: point the kernels at a [B][16] u64 stamp buffer.
int mc_debug_stamps(void* env, uint64_t* dev_stamps) {
  Env* E = as_env(env);
  if (!E) return fail(MC_EINVAL, "mc_debug_stamps: null env");
#if defined(MC_STAMPS) || defined(MC_DIST_STAMPS)
  E->s.stamps = dev_stamps;
  return MC_OK;
#else
  (void)dev_stamps;
  return fail(MC_EINVAL, "not a -DMC_STAMPS build");
#endif
}

int mc_check(void* env, void* stream) {
  Env* E = as_env(env);
  if (!E) return fail(MC_EINVAL, "mc_check: null env");
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(E->device));
  uint32_t err = 0;
  HIP_TRY(hipMemcpyAsync(&err, E->s.err, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (err) {
    HIP_TRY(hipMemsetAsync(E->s.err, 0, 4, st));
    HIP_TRY(hipStreamSynchronize(st));
    return fail(MC_EDEVICE,
                "device error word 0x%x (1=window 4=placement 8=inject 32=copy_envs index 64=export_maps index "
                "128=import_maps index or robots plane)",
                err);
  }
  return MC_OK;
}

}  // extern "C"
