// Stand-in for tinyxml2.h, ours.  The reference's Astar-3D/map.h includes tinyxml2.h (a leftover of the XML map reader
// of the library Astar-3D descends from) and uses nothing from it; the real header is not a dependency we carry.  This
// file only lets oracle/Makefile's `ref` target compile the reference's Astar-3D sources where they lie.  Standard
// includes only: the ones the reference's sources rely on getting through it.
#ifndef LSC_ORACLE_REF_STUB_TINYXML2_H
#define LSC_ORACLE_REF_STUB_TINYXML2_H
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#endif
