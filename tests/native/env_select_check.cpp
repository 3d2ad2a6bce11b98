// Stand-alone check of the env kernel's selection and launch geometry
// (csrc/mc_env_select.h), for a host-only build with sanitizers
// (tests/test_env_select_host.py builds and runs it; no HIP call).
//
// Every row of the list must be selected, by its label, by a State built from
// its own shape's fields; its public name must be the literal listed here;
// taking away what the row needs must fall back one step at a time; and the
// geometry rules must give tests/test_gpu_launch_shapes.py's ORGANIC table.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "mc_env_select.h"

static int fails = 0;
#define CHECK(c, ...)                     \
  do {                                    \
    if (!(c)) {                           \
      if (++fails <= 30) {                \
        std::printf("FAIL " __VA_ARGS__); \
        std::printf("\n");                \
      }                                   \
    }                                     \
  } while (0)

// what the rows must be, in order: label, public name, and the label of the
// march row a table row falls back to without a table (null: not a table row)
struct Want {
  const char *label, *name, *no_table;
};
static const Want kWant[] = {
    {"64,2,uint32_t,ShapeC2BV", "env_kernel<64,2,u32,C2>", "64,2,uint32_t,ShapeC2B"},
    {"64,2,uint32_t,ShapeC2V", "env_kernel<64,2,u32,C2>", "64,2,uint32_t,ShapeC2"},
    {"64,2,uint32_t,ShapeC2DV", "env_kernel<64,2,u32,C2D>", "64,2,uint32_t,ShapeC2D"},
    {"64,2,uint32_t,ShapeC2B", "env_kernel<64,2,u32,C2>", nullptr},
    {"64,2,uint32_t,ShapeC2", "env_kernel<64,2,u32,C2>", nullptr},
    {"64,2,uint32_t,ShapeC2D", "env_kernel<64,2,u32,C2D>", nullptr},
    {"64,1,uint32_t,ShapeC2V", "env_kernel<64,1,u32,C2>", "64,1,uint32_t,ShapeC2"},
    {"64,1,uint32_t,ShapeC2DV", "env_kernel<64,1,u32,C2D>", "64,1,uint32_t,ShapeC2D"},
    {"64,1,uint32_t,ShapeC2", "env_kernel<64,1,u32,C2>", nullptr},
    {"64,1,uint32_t,ShapeC2D", "env_kernel<64,1,u32,C2D>", nullptr},
    {"128,1,uint32_t,ShapeC5B", "env_kernel<128,1,u32,C5>", nullptr},
    {"128,1,uint32_t,ShapeC5", "env_kernel<128,1,u32,C5>", nullptr},
    {"256,1,uint64_t,ShapeC4B", "env_kernel<256,1,u64,C4>", nullptr},
    {"256,1,uint64_t,ShapeC4", "env_kernel<256,1,u64,C4>", nullptr},
    {"256,1,uint64_t,ShapeC4R", "env_kernel<256,1,u64,C4>", nullptr},
    {"64,2,uint32_t,Dynamic", "env_kernel<64,2,u32,generic>", nullptr},
    {"64,1,uint32_t,Dynamic", "env_kernel<64,1,u32,generic>", nullptr},
    {"128,1,uint32_t,Dynamic", "env_kernel<128,1,u32,generic>", nullptr},
    {"256,1,uint32_t,Dynamic", "env_kernel<256,1,u32,generic>", nullptr},
    {"512,1,uint32_t,Dynamic", "env_kernel<512,1,u32,generic>", nullptr},
    {"1024,1,uint32_t,Dynamic", "env_kernel<1024,1,u32,generic>", nullptr},
    {"64,2,uint64_t,Dynamic", "env_kernel<64,2,u64,generic>", nullptr},
    {"64,1,uint64_t,Dynamic", "env_kernel<64,1,u64,generic>", nullptr},
    {"128,1,uint64_t,Dynamic", "env_kernel<128,1,u64,generic>", nullptr},
    {"256,1,uint64_t,Dynamic", "env_kernel<256,1,u64,generic>", nullptr},
    {"512,1,uint64_t,Dynamic", "env_kernel<512,1,u64,generic>", nullptr},
    {"1024,1,uint64_t,Dynamic", "env_kernel<1024,1,u64,generic>", nullptr},
};
constexpr int kWantCount = (int)(sizeof(kWant) / sizeof(kWant[0]));

static const uint32_t kSomeTable[4] = {0, 0, 0, 0};  // what ray_prog / vis_tab point at when set (never read)

// a State that matches SH exactly and has what the row needs; a field the
// shape leaves open gets a value no compiled shape has
template <class SH>
static mc::State state_of(const mc::EnvRow& r) {
  mc::State s{};
  s.B = 8;
  s.G = 2;
  s.N = SH::N ? SH::N : 3;
  s.H = SH::H ? SH::H : (r.wbytes == 4 ? 5 : 13);
  s.TW = mc::window_tiles(s.H);
  s.sensor = 0;
  s.nbeams = SH::NB ? SH::NB : 9;
  s.ego = SH::EGO ? SH::EGO : 1;
  s.E = 2 * s.ego + 1;
  s.Lc = SH::LC;
  s.dist = SH::DS;
  s.beam_kmax = SH::KM ? SH::KM : 5;
  s.beam_kmin = SH::KN ? SH::KN : 4;
  s.fan_nsec = SH::FN;
  s.fan_nspec = SH::FS;
  s.fan_words = SH::FW;
  s.fan_kt = SH::FN ? SH::KM : 0;
  s.Wp = s.Lp = SH::BW ? SH::BW : 50;
  s.TR = s.TC = (s.Wp + 7) / 8;
  s.TRS = s.TCS = (s.TR + 3) / 4;
  s.MT = s.TRS * s.TCS * 16;
  s.auto_reset = 1;
  s.ray_prog = r.rayprog ? kSomeTable : nullptr;
  s.vis_tab = r.vistab ? kSomeTable : nullptr;
  return s;
}
using MakeState = mc::State(const mc::EnvRow&);
#define MAKER(T, P, W, SH, NAME) &state_of<mc::SH>,
static MakeState* const kMake[] = {MC_ENV_ROWS(MAKER)};

static const char* label_of(int i) { return i < 0 ? "(none)" : mc::kEnvRows[i].label; }
static std::string generic_of(const mc::EnvRow& r) {
  return std::to_string(r.nt) + "," + std::to_string(r.epw) + (r.wbytes == 4 ? ",uint32_t,Dynamic" : ",uint64_t,Dynamic");
}

static void check_rows() {
  CHECK(mc::kEnvRowCount == kWantCount, "%d rows, want %d", mc::kEnvRowCount, kWantCount);
  if (mc::kEnvRowCount != kWantCount) return;
  for (int i = 0; i < kWantCount; ++i) {
    const mc::EnvRow& r = mc::kEnvRows[i];
    const Want& w = kWant[i];
    CHECK(!std::strcmp(r.label, w.label), "row %d is %s, want %s", i, r.label, w.label);
    CHECK(!std::strcmp(r.name, w.name), "row %s is named %s, want %s", r.label, r.name, w.name);
    CHECK(r.vistab == (w.no_table != nullptr), "row %s: vistab %d", r.label, (int)r.vistab);
    // today's needs: C5 and generic rows nothing, C4 fits32, C2 also ray programs, C2 V rows also the table
    const bool c2 = std::strstr(r.label, "ShapeC2") != nullptr, c4 = std::strstr(r.label, "ShapeC4") != nullptr;
    CHECK(r.o32 == (c2 || c4) && r.rayprog == c2 && (!r.vistab || c2), "row %s needs o32 %d rayprog %d vistab %d",
          r.label, (int)r.o32, (int)r.rayprog, (int)r.vistab);
    const std::string gen = generic_of(r);

    mc::State s = kMake[i](r);
    CHECK(mc::env_fits32(s), "row %s: its own state does not fit 32 bits", r.label);
    int got = mc::select_env_row(s, r.nt, r.epw, true);
    CHECK(got == i, "row %s: its own state selects %s", r.label, label_of(got));
    // every C2 march row has a table row above it; no other shape reads a table
    CHECK(mc::env_takes_vis_table(s, r.nt, r.epw, true) == c2, "row %s: env_takes_vis_table", r.label);

    // the generic kernel without MARLCOV_SPECIALIZE
    got = mc::select_env_row(s, r.nt, r.epw, false);
    CHECK(gen == label_of(got), "row %s: spec off selects %s", r.label, label_of(got));
    CHECK(!mc::env_takes_vis_table(s, r.nt, r.epw, false), "row %s: a table with spec off", r.label);

    // maps past 32-bit offsets: by B, then by G
    for (int k = 0; k < 2; ++k) {
      mc::State t = s;
      (k ? t.G : t.B) = 1 << 24;
      CHECK(!mc::env_fits32(t), "row %s: large %s still fits 32 bits", r.label, k ? "G" : "B");
      got = mc::select_env_row(t, r.nt, r.epw, true);
      CHECK(r.o32 ? gen == label_of(got) : got == i, "row %s: large %s selects %s", r.label, k ? "G" : "B",
            label_of(got));
    }

    // the fallback chain, one step at a time
    if (r.vistab) {
      s.vis_tab = nullptr;
      got = mc::select_env_row(s, r.nt, r.epw, true);
      CHECK(!std::strcmp(w.no_table, label_of(got)), "row %s: no table selects %s", r.label, label_of(got));
      CHECK(mc::env_takes_vis_table(s, r.nt, r.epw, true), "row %s: would take a table", r.label);
    }
    if (r.rayprog) {
      s.ray_prog = nullptr;
      got = mc::select_env_row(s, r.nt, r.epw, true);
      CHECK(gen == label_of(got), "row %s: no ray programs selects %s", r.label, label_of(got));
      CHECK(!mc::env_takes_vis_table(s, r.nt, r.epw, true), "row %s: a table without ray programs", r.label);
    }
  }
  // a C2 state on two waves: no compiled row of that lane count
  {
    const mc::EnvRow& r = mc::kEnvRows[8];  // 64,1,uint32_t,ShapeC2
    const mc::State s = state_of<mc::ShapeC2>(r);
    CHECK(mc::select_env_row(s, 64, 1, true) == 8, "C2 at 64 lanes");
    const int got = mc::select_env_row(s, 128, 1, true);
    CHECK(!std::strcmp(label_of(got), "128,1,uint32_t,Dynamic"), "C2 at 128 lanes selects %s", label_of(got));
  }
  std::printf("rows %d\n", kWantCount);
}

// tests/test_gpu_launch_shapes.py ORGANIC: robots, beams (0: the square
// sensor), sensor range -> lanes, envs per workgroup, row word bytes
struct Organic {
  const char* name;
  int n, beams, range, nt, epw, wbytes;
};
static const Organic kOrganic[] = {
    {"wg512_u64_n12_r27", 12, 13, 27, 512, 1, 8},
    {"wg512_u64_n16_r27_edge", 16, 13, 27, 512, 1, 8},
    {"wg1024_u64_n17_r27", 17, 13, 27, 1024, 1, 8},
    {"wg1024_u64_n20_r27_ldsmax", 20, 13, 27, 1024, 1, 8},
    {"wg1024_u64_n30_r19_tw6", 30, 9, 19, 1024, 1, 8},
    {"wg512_u32_n64_r10", 64, 7, 10, 512, 1, 4},
    {"wg256_u32_n32_r8", 32, 9, 8, 256, 1, 4},
    {"square_r12_u64_packed", 2, 0, 12, 64, 2, 8},
    {"square_r9_u32_tw4", 3, 0, 9, 64, 2, 4},
    {"square_r12_n20_wg256", 20, 0, 12, 256, 1, 8},
    {"square_r27_n9_wg512", 9, 0, 27, 512, 1, 8},
    {"square_r11_n40_wg512_u32", 40, 0, 11, 512, 1, 4},
};

static mc::State organic_state(const Organic& o) {
  mc::State s{};
  s.B = 2;
  s.G = 2;
  s.N = o.n;
  s.H = o.range;  // max(ceil(range), egoradius): the range, in every case
  s.TW = mc::window_tiles(s.H);
  s.sensor = o.beams ? 0 : 1;
  s.nbeams = o.beams;
  s.MT = 16 * 9;
  return s;
}

static void check_geometry() {
  int n = 0;
  for (const Organic& o : kOrganic) {
    const mc::State s = organic_state(o);
    const mc::EnvGeom g = mc::env_geometry(s, 0);
    CHECK(g.nt == o.nt && g.epw == o.epw, "%s: <%d,%d>, want <%d,%d>", o.name, g.nt, g.epw, o.nt, o.epw);
    const int got = mc::select_env_row(s, g.nt, g.epw, true);
    const mc::EnvRow want{o.nt, o.epw, o.wbytes, false, false, false, false, nullptr, nullptr, nullptr};
    CHECK(generic_of(want) == label_of(got), "%s: selects %s", o.name, label_of(got));
    ++n;
  }
  // MARLCOV_NT: a value below the computed one, or none of 64 .. 1024, is
  // ignored; one above raises the lanes and leaves one env per workgroup
  const mc::State wide = organic_state(kOrganic[6]), packed = organic_state(kOrganic[8]);
  const struct { const mc::State* s; int ov, nt, epw; } kNt[] = {
      {&wide, 128, 256, 1}, {&wide, 256, 256, 1}, {&wide, 1024, 1024, 1}, {&wide, 300, 256, 1}, {&wide, 2048, 256, 1},
      {&packed, 0, 64, 2},  {&packed, 64, 64, 2}, {&packed, 128, 128, 1}, {&packed, 512, 512, 1}, {&packed, 100, 64, 2},
  };
  for (const auto& c : kNt) {
    const mc::EnvGeom g = mc::env_geometry(*c.s, c.ov);
    CHECK(g.nt == c.nt && g.epw == c.epw, "MARLCOV_NT=%d: <%d,%d>, want <%d,%d>", c.ov, g.nt, g.epw, c.nt, c.epw);
  }
  std::printf("geometry %d\n", n);
}

int main() {
  check_rows();
  check_geometry();
  if (fails) {
    std::printf("%d checks failed\n", fails);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
