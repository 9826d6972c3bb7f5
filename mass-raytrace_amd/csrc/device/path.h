// path.h — the device-side restatement of the reference's hot path for
// gfx950, by concern: surface.h, isect.h, walk.h, walk_nf.h, material.h.
#pragma once
#include "material.h"
#include "walk_nf.h"
