// Tile sizes of the all-pairs Stein kernels (stein.hip). vi_normflows_amd/ops/stein.py reads the
// two numbers from this file (TILE_I / TILE_J there), so the tests can place N around them.
#pragma once

#define NF_STEIN_TILE_I 128  // rows i per workgroup
#define NF_STEIN_TILE_J 64   // rows j staged in LDS at a time
