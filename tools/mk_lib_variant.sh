#!/bin/bash
# a full build of the library under extra compiler switches -> flash_hash_join_amd/lib/ab/<name>.so (loaded with FJ_LIB_VARIANT=<name>):
#   tools/mk_lib_variant.sh <name> -DFJ_LAB [-DFJ_WIDE_BS=8 ...]
# The objects are csrc/Makefile's SRCS, one per source, in a directory of the variant's own: make expands the list, none is kept here.
cd "$(dirname "$0")/../flash_hash_join_amd/csrc" || exit 1
name=$1; shift
mkdir -p ../lib/ab /tmp/fjv_$name
make -s -j${JOBS:-4} OUT=../lib/ab/$name.so 'OBJS=$(SRCS:%.hip=$(VARIANT_DIR)/%.o)' EXTRA="$*" VARIANT_DIR=/tmp/fjv_$name variant && echo "built lib/ab/$name.so"
