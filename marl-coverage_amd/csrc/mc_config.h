// mc_config.h — mc_create's pure half (mc_capi.hip): the checks of an
// mc_config and the State fields that follow from it alone.  Host-only, no
// HIP call, no environment read.
#pragma once
#include <math.h>
#include <stdint.h>

#include <string>

#include "marlcov.h"
#include "mc_internal.h"
#include "mc_msg.h"

namespace mc {

// Window half-width H of a config that check_config accepts: the sensor's
// reach or the obs crop's, whichever is larger.
inline int window_half(const mc_config& c) {
  // every marked cell is within Chebyshev ceil(range) of the robot: the
  // major axis moves exactly 1 per step and the fp64 distance sum of
  // increments >= 1 reaches range after at most ceil(range) steps
  const int hs = c.sensor_type != MC_SENSOR_LIDAR ? c.square_radius : (c.lidar_range > 0 ? (int)ceil(c.lidar_range) : 0);
  return hs > c.egoradius ? hs : c.egoradius;
}

// The first failing check decides the message (`err`); true: the config is one
// the kernels can run.
inline bool check_config(const mc_config& c, std::string& err) {
  const bool lidar = c.sensor_type == MC_SENSOR_LIDAR;
  if (c.num_envs < 1) return msgf(err, "num_envs must be >= 1 (got %d)", c.num_envs);
  if (c.num_agents < 1 || c.num_agents > 64) return msgf(err, "numrobot must be in [1, 64] (got %d)", c.num_agents);
  if (c.width < 3 || c.length < 3 || c.width > 32767 || c.length > 32767)
    return msgf(err, "padded grid %dx%d out of range", c.width, c.length);
  if (c.num_grids < 1) return msgf(err, "num_grids must be >= 1");
  if (!lidar && c.sensor_type != MC_SENSOR_SQUARE) return msgf(err, "unknown sensor_type %d", c.sensor_type);
  if (lidar && c.num_beams < 1) return msgf(err, "num_lasers must be >= 1");
  if (!lidar && c.square_radius < 0) return msgf(err, "square sensor range must be >= 0");
  if (c.egoradius < 0) return msgf(err, "egoradius must be >= 0");
  if (c.pad < c.egoradius) return msgf(err, "pad must be >= egoradius");
  if (c.mini_map_rad < 0 || c.pad < c.mini_map_rad) return msgf(err, "need 0 <= mini_map_rad <= pad");
  if (c.mini_map_rad > 0 && 2 * c.egoradius + 1 > 32) return msgf(err, "minimap layers need egoradius <= 15");
  if (!(c.lidar_range == c.lidar_range)) return msgf(err, "lidar range is NaN");
  if (c.maxsteps < 0) return msgf(err, "maxsteps must be >= 0");
  if (lidar && c.lidar_range > 31) return msgf(err, "lidar range %g > 31 not supported", c.lidar_range);
  const int H = window_half(c), TW = window_tiles(H);
  if (2 * c.egoradius + 1 > 32) return msgf(err, "egoradius %d > 15: obs crop rows are 32-bit", c.egoradius);
  if ((int64_t)c.num_agents * TW * TW > (int64_t)kMaxItemsPerLane * 1024)
    return msgf(err, "numrobot * %d^2 window tiles = %d exceeds %d (range/egoradius too large)", TW,
                c.num_agents * TW * TW, kMaxItemsPerLane * 1024);
  // the kernels index maps with 32-bit words and 24-bit factors
  const int64_t tiles = (int64_t)(((c.width + 7) / 8 + 3) / 4) * (((c.length + 7) / 8 + 3) / 4) * 16;
  if ((int64_t)c.num_envs * c.num_agents * tiles >= ((int64_t)1 << 32) ||
      (int64_t)c.num_envs * c.num_agents >= ((int64_t)1 << 24) || tiles >= ((int64_t)1 << 24))
    return msgf(err, "num_envs * numrobot * map tiles = %lld exceeds 2^32 words per handle",
                (long long)c.num_envs * c.num_agents * tiles);
  if (TW > kMaxWindowTiles) return msgf(err, "window half-width H = %d > 27 (range/egoradius too large)", H);
  if (env_lds_bytes(c.num_agents, TW, lidar ? c.num_beams : 0, TW <= 4 ? 4 : 8) > 65536)
    return msgf(err, "per-env LDS window exceeds 64 KiB (numrobot / range / num_lasers too large)");
  return true;
}

// The geometry, magic-division and flag fields of the State of an accepted config.
inline void derive_state(const mc_config& c, State& s) {
  s.B = c.num_envs;
  s.N = c.num_agents;
  s.Wp = c.width;
  s.Lp = c.length;
  s.TR = (c.width + 7) / 8;
  s.TC = (c.length + 7) / 8;
  s.TRS = (s.TR + 3) / 4;
  s.TCS = (s.TC + 3) / 4;
  s.MT = s.TRS * s.TCS * 16;
  s.G = c.num_grids;
  s.H = window_half(c);
  s.TW = window_tiles(s.H);
  s.mg_TW = magic_div((uint32_t)s.TW);
  s.mg_TW2 = magic_div((uint32_t)(s.TW * s.TW));
  s.ego = c.egoradius;
  s.pad = c.pad;
  s.E = 2 * c.egoradius + 1;
  s.Lc = (c.mini_map_rad > 0 ? 5 : 3) + (c.dist_reward ? 1 : 0) + (c.dijkstra_input ? 1 : 0);
  s.dist = c.dist_reward ? 1 : 0;
  s.mg_LcE = magic_div((uint32_t)(s.Lc * s.E));
  s.mg_E = magic_div((uint32_t)s.E);
  s.sensor = c.sensor_type;
  s.nbeams = c.sensor_type == MC_SENSOR_LIDAR ? c.num_beams : 0;
  s.mg_nb = magic_div((uint32_t)(s.nbeams > 0 ? s.nbeams : 1));
  s.sq_r = c.square_radius;
  s.pen = c.collision_penalty;
  s.term = c.terminal_reward;
  s.dincr = c.done_incr;
  s.maxsteps = c.maxsteps;
  s.comm_r = c.comm_radius;
  s.sst = c.single_square_tool ? 1 : 0;
  s.auto_reset = c.auto_reset ? 1 : 0;
  s.grid_mode = c.reset_grid_mode;
  s.seed = c.seed;
  s.env0 = c.env_offset;
  s.grid0 = c.grid_offset;
}

}  // namespace mc
