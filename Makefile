# Builds the gfx950 product library (hipcc) and the CPU oracle (gcc, test infra).
# -ffp-contract=off and no fast-math on every compile: the HIP kernels and the
# oracle must round identically.
HIPCC   ?= /opt/rocm/bin/hipcc
ARCH    ?= gfx950
PKG     := mc-path-tracer_amd
BUILD   := $(PKG)/build
# A/B variants (tools/build_variant.sh, build_rev*.sh): the library's name and extra compile flags
LIB     ?= mcpt
EXTRA_HIPFLAGS ?=
HIPFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math \
            -fhip-fp32-correctly-rounded-divide-sqrt -Wall -Wno-unused-function -Iinclude -I$(PKG)/csrc $(EXTRA_HIPFLAGS)
SRCS := $(PKG)/csrc/kernels.hip $(PKG)/csrc/scene_tables.hip $(PKG)/csrc/film.hip $(PKG)/csrc/bvh_build.hip $(PKG)/csrc/env_build.hip $(PKG)/csrc/denoise.hip $(PKG)/csrc/adaptive.hip $(PKG)/csrc/temporal.hip $(PKG)/csrc/variance.hip $(PKG)/csrc/refit.hip $(PKG)/csrc/emitter.hip $(PKG)/csrc/texture.hip $(PKG)/csrc/runtime.cpp $(PKG)/csrc/film_state.cpp $(PKG)/csrc/stage_run.cpp $(PKG)/csrc/scene_upload.cpp $(PKG)/csrc/postprocess.cpp \
        $(PKG)/csrc/host/scene.cpp $(PKG)/csrc/host/proxies.cpp $(PKG)/csrc/host/capi_host.cpp $(PKG)/csrc/host/pair_tree.cpp \
        $(PKG)/csrc/host/image_io.cpp $(PKG)/csrc/host/emitter_table.cpp $(PKG)/csrc/host/tangents.cpp \
        $(PKG)/csrc/host/png_read.cpp
OBJS := $(patsubst $(PKG)/csrc/%,$(BUILD)/%.o,$(SRCS))
HDRS := include/mcpt.h $(PKG)/csrc/kernels.hpp $(PKG)/csrc/device/mcpt_core.hpp $(PKG)/csrc/device/scene_dev.hpp \
        $(PKG)/csrc/device/primary_beam.hpp $(PKG)/csrc/device/occ_beam.hpp $(PKG)/csrc/device/denoise.hpp $(PKG)/csrc/device/adaptive.hpp $(PKG)/csrc/device/temporal.hpp $(PKG)/csrc/device/variance.hpp $(PKG)/csrc/device/texture.hpp $(PKG)/csrc/device/srgb_table.hpp $(PKG)/csrc/device/k_material_body.inc \
        $(PKG)/csrc/runtime_internal.hpp $(PKG)/csrc/host/host_internal.hpp $(PKG)/csrc/host/pair_tree.hpp \
        $(PKG)/csrc/host/emitter_table.hpp $(PKG)/csrc/host/film_layout.hpp

all: $(PKG)/libmcpt.so oracle/liboracle.so examples/mcpt_render tests/native/facade_test tests/native/primary_beam tests/native/occ_beam tests/native/emitter_table_host \
     tests/native/env_search_host tests/native/env_search_host_san tests/native/srgb_table_host

$(BUILD)/%.o: $(PKG)/csrc/% $(HDRS)
	@mkdir -p $(dir $@)
	$(HIPCC) $(HIPFLAGS) -x hip -c $< -o $@

$(PKG)/lib$(LIB).so: $(OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(OBJS)

# C++ example over the C ABI only: render a BASELINE config, write PNG/PFM
examples/mcpt_render: examples/mcpt_render.cpp include/mcpt.h $(PKG)/libmcpt.so
	g++ -O2 -std=c++17 -Iinclude $< -L$(PKG) -lmcpt -Wl,-rpath,'$$ORIGIN/../$(PKG)' -o $@

example: examples/mcpt_render

# C++ host facade (include/mcpt.hpp) test driver: host checks on the CPU, a config-1 render on the GPU
tests/native/facade_test: tests/native/facade_test.cpp include/mcpt.hpp include/mcpt.h $(PKG)/libmcpt.so
	g++ -O2 -std=c++17 -Wall -Wextra -Iinclude $< -L$(PKG) -lmcpt -Wl,-rpath,'$$ORIGIN/../../$(PKG)' -o $@

# Host check of the primary beam's interval bounds (device/primary_beam.hpp) on the CPU
tests/native/primary_beam: tests/native/primary_beam.cpp $(PKG)/csrc/device/primary_beam.hpp $(PKG)/csrc/device/mcpt_core.hpp
	$(HIPCC) -O2 -std=c++17 -ffp-contract=off -fno-fast-math -Iinclude -I$(PKG)/csrc $< -o $@

# Host check of the occluder table's complete candidate lists (device/occ_beam.hpp) on the CPU
tests/native/occ_beam: tests/native/occ_beam.cpp $(PKG)/csrc/device/occ_beam.hpp $(PKG)/csrc/device/primary_beam.hpp $(PKG)/csrc/device/mcpt_core.hpp
	$(HIPCC) -O2 -std=c++17 -ffp-contract=off -fno-fast-math -Iinclude -I$(PKG)/csrc $< -o $@

# Host check of the emitter table builder (host/emitter_table.cpp) as a stand-alone CPU program
tests/native/emitter_table_host: tests/native/emitter_table_host.cpp $(PKG)/csrc/host/emitter_table.cpp $(PKG)/csrc/host/emitter_table.hpp
	g++ -O2 -std=c++17 -Wall -Wextra -ffp-contract=off -I$(PKG)/csrc $< $(PKG)/csrc/host/emitter_table.cpp -o $@

# Host check of the env light's guided CDF search against the plain bisection (device/mcpt_core.hpp) on the
# CPU, and the same program under the host sanitizers (run directly: it loads nothing else)
tests/native/env_search_host: tests/native/env_search_host.cpp $(PKG)/csrc/device/mcpt_core.hpp
	$(HIPCC) -O2 -std=c++17 -ffp-contract=off -fno-fast-math -Iinclude -I$(PKG)/csrc $< -o $@
tests/native/env_search_host_san: tests/native/env_search_host.cpp $(PKG)/csrc/device/mcpt_core.hpp
	$(HIPCC) -O1 -g -std=c++17 -ffp-contract=off -fno-fast-math -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
	    -Iinclude -I$(PKG)/csrc $< -o $@

# Host reader of the sRGB table and lookup (device/texture.hpp) on the CPU
tests/native/srgb_table_host: tests/native/srgb_table_host.cpp $(PKG)/csrc/device/texture.hpp $(PKG)/csrc/device/srgb_table.hpp $(PKG)/csrc/device/mcpt_core.hpp
	$(HIPCC) -O2 -std=c++17 -ffp-contract=off -fno-fast-math -Iinclude -I$(PKG)/csrc $< -o $@


oracle/liboracle.so: oracle/mcpt_oracle.c oracle/trav_model.c oracle/mcpt_oracle.h
	$(MAKE) -C oracle

clean:
	rm -rf $(BUILD) $(PKG)/libmcpt.so examples/mcpt_render tests/native/facade_test tests/native/primary_beam tests/native/occ_beam tests/native/emitter_table_host \
	    tests/native/env_search_host tests/native/env_search_host_san tests/native/srgb_table_host
	$(MAKE) -C oracle clean

.PHONY: all clean
