// env.h — integer switches from the environment.
#pragma once

#include <cstdlib>

namespace quda {

// the value of `name`, dflt where it is unset; a switch that is read once keeps the result in a function-local static of its reader
inline int envInt(const char *name, int dflt) { const char *e = getenv(name); return e ? atoi(e) : dflt; }

}  // namespace quda
