// api_common.hpp — what the files that implement the C-ABI share: the calling thread's error string and the scene handle.
#pragma once
#include <string>

#include "../../include/doomgpu.h"
#include "scene.hpp"

extern thread_local std::string t_err;          // what dg_last_error reports (defined next to it, in api_scene.cpp)
inline int set_err(int code, const std::string &m) { t_err = m; return code; }

struct dg_scene { dg::Scene *sc; };
