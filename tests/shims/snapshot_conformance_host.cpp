// TEST INFRASTRUCTURE.  Host half of the snapshot API conformance check (see
// snapshot_conformance.inl): plain host C++, as a simulator's Manager is.
#define SNAPCONF_NAME snapconf_host
#include "snapshot_conformance.inl"
