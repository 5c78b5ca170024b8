// sgp_stage_carve.h -- the regions of one call in the world's stage buffer (sgp_world::stage_host and stage_dev share one layout).  Host only and free of
// HIP types, so that tests/cpp/stage_carve_check.cpp can exercise it under a sanitizer without a GPU.
#pragma once
#include <stddef.h>

struct StageCarve {
	size_t total = 0;      // the end of the last region: what ensure_stage is asked for
	// appends a region of `bytes` at the next 16-byte boundary and returns its offset
	size_t add(size_t bytes) { const size_t off = (total + 15) & ~size_t(15); total = off + bytes; return off; }
	// a region in one of the two buffers
	template <class T> static T* at(void* base, size_t off) { return (T*)((char*)base + off); }
};
