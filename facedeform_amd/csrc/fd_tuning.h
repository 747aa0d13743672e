// fd_tuning.h -- the one place environment variables are read.
#pragma once
// Diagnostic instruments (FD_REG_STAMPS, FD_SMALL_STAMPS, FD_SHARED_STAMPS, FD_COOK_TIMING) are environment variables ONLY in
// tuning builds (-DFD_TUNING: tools/, profile collections); the product library reads no environment variable -- a library that
// lives inside Houdini does not change its behaviour by the environment of the process that loaded it.
// Per-context choices go through fd_config.
#include <cstdlib>
#ifdef FD_TUNING
static inline const char *tuning_env(const char *name) { return getenv(name); }
#else
static inline const char *tuning_env(const char *) { return nullptr; }
#endif

