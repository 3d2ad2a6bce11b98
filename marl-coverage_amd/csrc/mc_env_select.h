// mc_env_select.h — which env-kernel instantiation runs a State: the compiled
// shapes, an instantiation's compile-time configuration (EnvCfg), the list of
// instantiations (MC_ENV_ROWS) and the launch geometry.  Plain host code, no
// HIP call and no getenv: tests/native/env_select_check.cpp runs it as it is.
//
// The list is expanded twice: here into kEnvRows (what select_env_row walks)
// and in mc_env_kernel.hip into the launchers, so row i of one is row i of the
// other.  The files mc_env_inst_*.hip expand one group each into explicit
// instantiations of launch_one (mc_env_step.h).
#pragma once
#include <type_traits>

#include "mc_internal.h"
#include "mc_vistab.h"

namespace mc {

// ---- the compiled shapes (ShapeNone, mc_internal.h), each as its difference
// from its parent
struct ShapeC2 : ShapeNone {  // the bench workload
  static constexpr int N = 4, H = 10, NB = 21, EGO = 2, KM = 10, KN = 8;
};
struct ShapeC2D : ShapeC2 { static constexpr int LC = 4; };  // C2 + dijkstra_input (4 obs layers)
// 360 beams, R=20, marched by rays (MARLCOV_FAN=0) ...
struct ShapeC4R : ShapeNone {
  static constexpr int N = 8, H = 20, NB = 360, EGO = 2, KM = 20, KN = 15;
};
// ... and with its fan baked in: 64 sector slots, 2 special beams, 1,024 LUT
// words + 32 pair records x 42 + 2 x 8 = 2,384 words
struct ShapeC4 : ShapeC4R { static constexpr int FN = 64, FS = 2, FW = 2384; };
// 16 agents, egoradius 2, dist_reward (4 obs layers)
struct ShapeC5 : ShapeC2 { static constexpr int N = 16, LC = 4, DS = 1; };
// the bench instantiations (bench.py CONFIGS: 128x128 / 256x256 / 512x512
// grids, auto-reset, no comm graph); other grids run the shapes above
struct ShapeC2B : ShapeC2 { static constexpr int BW = 130; };
struct ShapeC4B : ShapeC4 { static constexpr int BW = 258; };
struct ShapeC5B : ShapeC5 { static constexpr int BW = 514; };
// the C2 shapes with the lidar's marks read from the visibility table (EnvCfg::VISTAB)
struct ShapeC2V : ShapeC2 { static constexpr int VT = 1; };
struct ShapeC2DV : ShapeC2D { static constexpr int VT = 1; };
struct ShapeC2BV : ShapeC2B { static constexpr int VT = 1; };

// whether a compile-time obs shape takes write_obs_fast (mc_env_step.h)
template <int EGO, int NS, int LC = 3>
struct ObsFast {
  static constexpr int E = 2 * EGO + 1, EE = E * E, NB = LC * NS;
  static constexpr bool ok = EGO > 0 && NS > 0 && EE <= 28 && (NB * EE) % 4 == 0 && (LC == 3 || LC == 4);
};

// Which (agent, tile) items a lane stages, where the shape fixes it: item k of
// lane `sub` of an env slot of LPE lanes is number idx = sub + k * LPE of the
// N * TW * TW items, agent idx / TW^2, tile (ti, tj) = (idx % TW^2 / TW,
// idx % TW).  With TW^2 a power of two that divides LPE these are bit fields
// of the lane id and constants of k (stage_load's general form divides twice
// per item and step), and item k is live in every lane or in none.
template <int LPE, int N, int TW>
struct ItemGeo {
  static constexpr int TW2 = TW * TW;
  static constexpr int AG = TW2 > 0 ? LPE / TW2 : 0;  // agents one item round of the slot covers
  static constexpr bool ok = N > 0 && TW > 0 && (TW & (TW - 1)) == 0 && LPE % TW2 == 0 && (AG & (AG - 1)) == 0 &&
                             (N * TW2) % LPE == 0;
  __host__ __device__ static constexpr bool live(int k) { return k * LPE < N * TW2; }
  // the agents item k can belong to: first(k) .. first(k) + AG - 1
  __host__ __device__ static constexpr int first(int k) { return k * AG; }
  __host__ __device__ static constexpr int agent(int sub, int k) {  // (a dead item: agent 0, as stage_load has it)
    return live(k) ? first(k) + (int)(((uint32_t)sub / (uint32_t)TW2) & (uint32_t)(AG - 1)) : 0;
  }
  __host__ __device__ static constexpr int ti(int sub) { return (int)(((uint32_t)sub / (uint32_t)TW) & (uint32_t)(TW - 1)); }
  __host__ __device__ static constexpr int tj(int sub) { return (int)((uint32_t)sub & (uint32_t)(TW - 1)); }
};

// Everything fixed at compile time for one env_kernel<NT, EPW, WT, SH>
// instantiation (the kernel's Ctx derives from it, mc_env_step.h).  O32,
// RAYPROG and VISTAB are also what the instantiation asks of a State before
// select_env_row takes it.
template <int NT_, int EPW_, typename WT_, class SH_>
struct EnvCfg {
  using WT = WT_;  // a window row's word (u32: TW <= 4, else u64)
  using SH = SH_;  // the compiled shape (Dynamic: nothing baked in)
  static constexpr int NT = NT_, EPW = EPW_;      // workgroup lanes, envs per workgroup
  static constexpr int LPE = NT / EPW;            // lanes per env
  static constexpr int KI = kMaxItemsPerLane;     // staged tiles per lane
  static constexpr int RPL0 = ray_rpl0(EPW);      // beams per lane per pass (mc_internal.h)
  static constexpr int KM = SH::KM, KN = SH::KN;  // the shape's beam_kmax (fan trip count) and beam_kmin; 0: runtime
  // march steps per batch: the whole march when the shape fixes a short
  // beam_kmax, a quarter of a long one (register pressure)
  static constexpr int SUK0 = (SH::KM > 0 && SH::KM <= 12) ? SH::KM : (SH::KM > 12 ? (SH::KM + 3) / 4 : 8);
  // compile-time agent count, if small (merge, the register front); the
  // moves, dist_window_am2 and the obs read SH::N under bounds of their own
  static constexpr int NSM = (SH::N > 0 && SH::N <= 8) ? SH::N : 0;
  // rays per lane per march pass: 3 where that saves a pass over the
  // default (C5: 336 rays over 128 lanes, one pass of 3 instead of two of 2)
  static constexpr int RPLK = ray_rplk(NT, EPW, SH::N, SH::NB);
  static constexpr int RPL = ray_rpl(NT, EPW, SH::N, SH::NB);
  // (3 rays per lane: half the march's batch, the row words of a batch stay
  // within the register budget)
  static constexpr int SUK = RPLK == 3 ? (SUK0 + 1) / 2 : SUK0;
  // compiled shapes with up to 8 agents: map byte offsets fit 32 bits
  // (select_env_row checks env_fits32; the C5 shape's maps pass 4 GB)
  static constexpr bool O32 = SH::N > 0 && SH::N <= 8;
  // register front (front_regs / moves_front): compiled agent count <= 8, one wave per workgroup
  static constexpr bool FRONT = NSM > 0 && NT == 64;
  // moves from registers in the first wave of a multi-wave env during round
  // trip 2 (compiled agent count <= 8, lidar: C4)
  static constexpr bool EARLY = NSM > 0 && NT > 64 && EPW == 1 && SH::NB > 0;
  // dist_reward: lane i < N loads its agent's PRE terms right after the moves
  // (compiled shapes; the generic kernels keep the loads in the reward:
  // two more live registers there cost the u64 ones a wave per SIMD)
  static constexpr bool kPrePrefetch = SH::N > 0;
  // the obs: write_obs_fast for a compile-time obs shape whose crops fit the
  // first wave, else write_obs with the robots in registers up to 16 agents
  static constexpr bool OBS_FAST = ObsFast<SH::EGO, SH::N, SH::LC>::ok && (NT == 64 || EPW == 1) &&
                                   ObsFast<SH::EGO, SH::N, SH::LC>::NB <= 64;
  static constexpr int NS_OBS = (SH::N > 0 && SH::N <= 16) ? SH::N : 0;
  // the march from the host-built ray programs (mc_beams.h build_ray_prog;
  // select_env_row: State::ray_prog is set): compiled sparse-beam shapes of up
  // to 8 agents with one wave per workgroup whose rays take one pass -- no beam
  // records in LDS, no ray_init, no ray_advance chain.  Without a program
  // (beam patterns that depend on the start, or MARLCOV_BEAM_TABLE) the
  // generic kernel of the same geometry runs
  static constexpr bool RAYPROG = SH::NB > 0 && SH::NB < 64 && SH::KM > 0 && SH::KM <= 12 && NT == 64 && NSM > 0 &&
                                  sizeof(WT) == 4 && SH::N * SH::NB <= RPL * LPE;
  static constexpr int RPW = RAYPROG ? ray_prog_row_words(RPL, SH::KM) : 4;  // words of a lane's program row
  static_assert(!RAYPROG || ray_prog_span(SH::N, (int)sizeof(WT), SH::KM) <= 32767, "ray program offsets are int16");
  // a step's lidar marks from the visibility table (mc_vistab.h;
  // select_env_row: State::vis_tab is set, mc_capi.hip vis_refresh) instead of
  // the march: every (agent, tile) item loads its own tile of its robot's
  // record (vis_items), in a step and in a reset's initial sense alike -- such
  // a kernel holds no march at all
  static constexpr bool VISTAB = RAYPROG && SH::VT != 0 && vis_fits(SH::H);
  // the fused loop carries the lane's constants in registers (LaneK,
  // mc_env_step.h) instead of deriving them from the lane id in every step:
  // the one-wave kernels of the compiled shapes
  static constexpr bool LANEK = NT == 64 && NSM > 0;
  // the same kernels keep a staged tile's index in a register from stage_load
  // to store_tiles instead of computing it twice (two VGPRs per lane: the
  // C4 bench kernel, at 128, has none to give)
  static constexpr bool KEEP_GT = LANEK;
  // the fused loop also carries the env head (HeadK, mc_env_step.h: the robot
  // cells, the env's counters, the next step's action bytes) instead of loading
  // back what the wave stored a step earlier: the one-wave table kernels only
  // (the march rows have no VGPRs to give: 13 more words cost them a wave)
  static constexpr bool CARRY = LANEK && VISTAB;
  // ... and take their items' agents and tiles from the lane id (ItemGeo), run
  // the union dedup over the (item, lower agent) rounds that leaves and clip
  // the stored obstacle tiles with two masks (edge_clip, mc_internal.h)
  using GEO = ItemGeo<LPE, SH::N, window_tiles(SH::H)>;
  static_assert(!CARRY || GEO::ok, "the carried kernels' items are bit fields of the lane id");
};

// ---- the instantiations: X(NT, EPW, word, shape, public name), one row per
// kernel, in four groups (one mc_env_inst_*.hip each).  select_env_row takes
// the first row that fits, so among rows of one <NT, EPW, word> the order is
// the priority: table shapes before march shapes, bench shapes before general
// ones, the generic kernel last.  The public names (mc_kernel_variant) do not
// tell a bench or table shape from its general one; the labels do.
#define MC_ENV_ROWS_C2(X)                 \
  X(64, 2, uint32_t, ShapeC2BV, "u32,C2") \
  X(64, 2, uint32_t, ShapeC2V, "u32,C2")  \
  X(64, 2, uint32_t, ShapeC2DV, "u32,C2D") \
  X(64, 2, uint32_t, ShapeC2B, "u32,C2")  \
  X(64, 2, uint32_t, ShapeC2, "u32,C2")   \
  X(64, 2, uint32_t, ShapeC2D, "u32,C2D") \
  X(64, 1, uint32_t, ShapeC2V, "u32,C2")  \
  X(64, 1, uint32_t, ShapeC2DV, "u32,C2D") \
  X(64, 1, uint32_t, ShapeC2, "u32,C2")   \
  X(64, 1, uint32_t, ShapeC2D, "u32,C2D")
#define MC_ENV_ROWS_C45(X)                 \
  X(128, 1, uint32_t, ShapeC5B, "u32,C5") \
  X(128, 1, uint32_t, ShapeC5, "u32,C5")  \
  X(256, 1, uint64_t, ShapeC4B, "u64,C4") \
  X(256, 1, uint64_t, ShapeC4, "u64,C4")  \
  X(256, 1, uint64_t, ShapeC4R, "u64,C4")
#define MC_ENV_ROWS_GEN32(X)                  \
  X(64, 2, uint32_t, Dynamic, "u32,generic")  \
  X(64, 1, uint32_t, Dynamic, "u32,generic")  \
  X(128, 1, uint32_t, Dynamic, "u32,generic") \
  X(256, 1, uint32_t, Dynamic, "u32,generic") \
  X(512, 1, uint32_t, Dynamic, "u32,generic") \
  X(1024, 1, uint32_t, Dynamic, "u32,generic")
#define MC_ENV_ROWS_GEN64(X)                  \
  X(64, 2, uint64_t, Dynamic, "u64,generic")  \
  X(64, 1, uint64_t, Dynamic, "u64,generic")  \
  X(128, 1, uint64_t, Dynamic, "u64,generic") \
  X(256, 1, uint64_t, Dynamic, "u64,generic") \
  X(512, 1, uint64_t, Dynamic, "u64,generic") \
  X(1024, 1, uint64_t, Dynamic, "u64,generic")
#define MC_ENV_ROWS(X) MC_ENV_ROWS_C2(X) MC_ENV_ROWS_C45(X) MC_ENV_ROWS_GEN32(X) MC_ENV_ROWS_GEN64(X)

struct EnvRow {
  int nt, epw, wbytes;           // <NT, EPW, word>
  bool compiled;                 // not a generic kernel: MARLCOV_SPECIALIZE=0 skips it
  bool o32, rayprog, vistab;     // EnvCfg's: needs env_fits32, State::ray_prog, State::vis_tab
  bool (*matches)(const State&);
  const char* name;              // mc_kernel_variant
  const char* label;             // "NT,EPW,word,shape"
};
template <int T, int P, typename W, class SH>
constexpr EnvRow env_row(const char* name, const char* label) {
  using C = EnvCfg<T, P, W, SH>;
  return {T, P, (int)sizeof(W), !std::is_same_v<SH, Dynamic>, C::O32, C::RAYPROG, C::VISTAB, &shape_matches<SH>,
          name, label};
}
#define MC_ENV_ROW(T, P, W, SH, NAME) env_row<T, P, W, SH>("env_kernel<" #T "," #P "," NAME ">", #T "," #P "," #W "," #SH),
inline constexpr EnvRow kEnvRows[] = {MC_ENV_ROWS(MC_ENV_ROW)};
#undef MC_ENV_ROW
constexpr int kEnvRowCount = (int)(sizeof(kEnvRows) / sizeof(kEnvRows[0]));

// an O32 kernel addresses the map arrays with 32-bit byte offsets
inline bool env_fits32(const State& s) {
  const uint64_t mtb = (uint64_t)s.MT * 8;
  return (uint64_t)s.B * s.N * mtb < (1ull << 32) && (uint64_t)s.G * mtb < (1ull << 32);
}

// The row for this state, lane count and envs per workgroup: the first whose
// <NT, EPW, word> is the launch's (u32 rows when TW <= 4), whose needs the
// State meets and whose shape matches it exactly -- a compiled shape, else the
// generic kernel.  spec: compiled shapes may run (MARLCOV_SPECIALIZE).
// has_tab: whether the State counts as having a visibility table.
inline int env_row_for(const State& s, int nt, int epw, bool spec, bool has_tab) {
  if (epw == 2) nt = 64;  // two envs per workgroup share one wave
  const int wbytes = s.TW <= 4 ? 4 : 8;
  const bool fits32 = env_fits32(s);
  for (int i = 0; i < kEnvRowCount; ++i) {
    const EnvRow& r = kEnvRows[i];
    if (r.nt != nt || r.epw != epw || r.wbytes != wbytes || (r.compiled && !spec)) continue;
    if ((r.o32 && !fits32) || (r.rayprog && !s.ray_prog) || (r.vistab && !has_tab)) continue;
    if (r.matches(s)) return i;
  }
  return -1;  // no such launch geometry
}
inline int select_env_row(const State& s, int nt, int epw, bool spec) {
  return env_row_for(s, nt, epw, spec, s.vis_tab != nullptr);
}
// whether a step of this state would read the visibility table if the handle
// had one (mc_capi.hip builds it only then)
inline bool env_takes_vis_table(const State& s, int nt, int epw, bool spec) {
  const int i = env_row_for(s, nt, epw, spec, true);
  return i >= 0 && kEnvRows[i].vistab;
}

// ---- launch geometry
// Lanes of an env's workgroup: every lane stages at most kMaxItemsPerLane
// (agent, tile) items; beyond that, prefer one wave per env (no cross-wave
// barriers) unless the beam march would need more than ~8 sequential rounds
// per lane
inline int env_threads(const State& s) {
  const int items = s.N * s.TW * s.TW;
  int nt = 64;
  while (nt < 1024 && items > kMaxItemsPerLane * nt) nt *= 2;
  if (s.sensor == 0)
    while (nt < 256 && s.N * s.nbeams > 8 * nt) nt *= 2;
  return nt;
}
// Envs per wave: two when an env fits 32 lanes (N <= 32, at most KI staged
// tiles and 3 beams per lane), else one env per workgroup of NT threads.
inline int env_pack(const State& s) {
  const int items = s.N * s.TW * s.TW;
  const int rays = s.sensor == 0 ? s.N * s.nbeams : 0;
  return (s.N <= 32 && items <= kMaxItemsPerLane * 32 && rays <= 3 * 32) ? 2 : 1;
}
// Lanes per workgroup and envs per workgroup of a State.  nt_override
// (MARLCOV_NT, 0: none; a tuning / test knob): 64 .. 1024 can raise the lane
// count, never lower it; more than one wave leaves one env per workgroup
// (only the override gets there with a packable env).
struct EnvGeom {
  int nt, epw;
};
inline EnvGeom env_geometry(const State& s, int nt_override) {
  int nt = env_threads(s);
  const int v = nt_override;
  if ((v == 64 || v == 128 || v == 256 || v == 512 || v == 1024) && v > nt) nt = v;
  return {nt, nt > 64 ? 1 : env_pack(s)};
}

// One launch of env_kernel<T, P, W, SH> (defined in mc_env_step.h,
// instantiated by the mc_env_inst_*.hip files)
using EnvLauncher = void(const State& s, int mode, const uint8_t* actions, const uint8_t* env_mask,
                         const int32_t* inj_pos, double* reward, uint8_t* done, uint8_t* obs, uint8_t* adj,
                         int num_steps, const EnvStrides& strides, hipStream_t stream);
template <int T, int P, typename W, class SH>
EnvLauncher launch_one;

}  // namespace mc
