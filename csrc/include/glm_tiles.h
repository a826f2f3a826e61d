// Tile sizes of the GLM likelihood kernel (glm.hip). vi_normflows_amd/ops/glm.py reads the two
// numbers from this file (TILE_B / TILE_N there), so the tests can place B and N around them.
#pragma once

#define NF_GLM_TILE_B 128  // rows of theta per workgroup
#define NF_GLM_TILE_N 64   // data rows [x_n | y_n] staged in LDS at a time
